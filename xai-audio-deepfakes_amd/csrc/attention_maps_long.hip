// Attention maps, the AH-rule's value-only backward and rollout for clips of any length and per-clip lengths: the streamed forms of
// advh_attention_maps / advh_rollout_step / advh_rollout_relevance (attention_maps.hip) and advh_attention_bwd_value (lrp.hip),
// whose whole-clip kernels hold a (clip, head)'s keys in LDS and stop at T = 256 frames.
//
// The conventions are those of attention_bwd_long.hip: every product on v_mfma_f32_16x16x4_f32 for both operand formats (split
// plane pairs and plain fp16, lo == 0, joined to fp32 when staged: attention_f32_tiles.h), blocks of 128 rows aligned to row 0,
// eight wavefronts per workgroup, a nullable per-clip `frames` with Tv = clamp(frames[b], 1, T) while T stays the STRIDE, a
// workgroup whose block lies at or beyond Tv writes its zeros and returns before any barrier, no atomics and no scratch.  What is
// computed for a clip depends on Tv alone; rows >= Tv of qkv / dctx / the workspace are never read.
//
//   statistics kernel, grid (heads, B, ceil(T / 128)): sweep 1 of attention_bwd_long.hip's query kernel without dP and V.  The q
//     fragments of eight 16-query tiles sit in registers, K streams through LDS in blocks of 128; an online maximum m (log2 domain)
//     and sum l, rescaled by 2^(m_old - m_new) when a block raises the maximum; (m, 1 / l) go to planes 0 and 1 of the caller's
//     workspace, laid out as that file's stats[3][B * heads * T] (plane 2 is not touched).
//   maps kernel, grid (fuse ? 1 : heads, B, ceil(T / 128)^2): a workgroup owns one 128-query x 128-key tile of one clip's output,
//     a wavefront 16 queries x 128 keys with the scores TRANSPOSED (a lane's four registers of a tile are four consecutive keys of
//     one output row: 16-byte stores where T % 4 == 0).  P = exp2(s c2 - m) / l comes from the statistics: no pass over the other
//     key blocks.  The fused modes loop over the heads in index order, restage that head's K block (and V block in the gradient
//     form) and keep the fused tile in registers: one fold order, no [B, heads, T, T] intermediate.
//   value kernel, grid (heads, B, ceil(T / 128)): the key kernel of attention_bwd_long.hip without dK and dS.  A workgroup owns 128
//     keys (k fragments and the dV^T accumulators in registers) and streams Q and dO in blocks of 128 rows, in index order, with
//     those rows' (m, 1 / l); it zeroes the Q and K thirds of its own rows.
//   rollout step / relevance: the kernels of attention_maps.hip with every bound, the contraction loop included, at Tv.
//
// The scaled score is ONE rounded product at the three sites that form it (aml_score / aml_exponent restate bwl_score /
// bwl_exponent: contraction off), and S visits d in the order of MFMA4 on the same joined operands, so the P of the maps and value
// kernels is the exponential of exactly the score the statistics were taken over.
//
//   dynamic LDS   statistics: one fp32 matrix [128][D + 4];  maps: one (P) or two (gradient form);  value: two + 2 x 128 floats
//   D =  32        18 432 B |  18 432 /  36 864 B |  37 888 B
//   D =  64        34 816 B |  34 816 /  69 632 B |  70 656 B
//   D = 128        67 584 B |  67 584 / 135 168 B | 136 192 B
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"
#include "attention_f32_tiles.h"

namespace advh {

constexpr int AML_NW = 8;                          // wavefronts per workgroup: two per SIMD
constexpr int AML_RB = 16 * AML_NW;                // rows a workgroup owns (queries; keys in the value kernel)
constexpr int AML_SB = 128;                        // rows of a staged block
constexpr int AML_NTH = 64 * AML_NW;

constexpr int aml_lds_stats(int D) { return AML_SB * (D + 4) * 4; }
constexpr int aml_lds_maps(int D, bool grad) { return (grad ? 2 : 1) * AML_SB * (D + 4) * 4; }
constexpr int aml_lds_value(int D) { return (2 * AML_SB * (D + 4) + 2 * AML_SB) * 4; }

typedef _Float16 aml_h4 __attribute__((ext_vector_type(4)));

// bwl_score / bwl_exponent of attention_bwd_long.hip: the product is rounded before m is subtracted, at every site
__device__ __forceinline__ float aml_score(float s, float c2) {
#pragma clang fp contract(off)
    return s * c2;
}
__device__ __forceinline__ float aml_exponent(float s, float c2, float m) {
#pragma clang fp contract(off)
    const float t = s * c2;
    return t - m;
}

__device__ __forceinline__ int aml_valid_rows(const int* frames, int b, int T) {
    if (!frames) return T;
    const int f = frames[b];
    return f < 1 ? 1 : (f > T ? T : f);
}

// rows r0 <= t < r1 of one third of dqkv, this head's dm columns from `col0` on, <- 0 in every plane; dm % 8 == 0: 8-byte stores
__device__ __forceinline__ void aml_zero_rows(_Float16* dbase, long dqkv_lo, long ld, int col0, int r0, int r1, int dm, int tid) {
    const int c4 = dm / 4, n = (r1 - r0) * c4;
    for (int i = tid; i < n; i += AML_NTH) {
        const long o = (long)(r0 + i / c4) * ld + col0 + (i % c4) * 4;
        *(aml_h4*)(dbase + o) = aml_h4{0, 0, 0, 0};
        if (dqkv_lo) *(aml_h4*)(dbase + dqkv_lo + o) = aml_h4{0, 0, 0, 0};
    }
}

// ---------------------------------------------------------------------------------------------- statistics: (m, 1 / l) per query
template <int D>
__global__ __launch_bounds__(AML_NTH) void attention_stats_long_kernel(const _Float16* __restrict__ qkv, long qkv_lo, float* __restrict__ stats,
                                                                       long stats_plane, const int* __restrict__ frames, int T, int H, int dm,
                                                                       float scale) {
    constexpr int KB = AML_SB, NTB = KB / 16, PITCH = D + 4, DG = D / 16;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* Ks = smf;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * AML_RB;
    const int Tv = aml_valid_rows(frames, b, T);
    if (row0 >= Tv) return;                      // workgroup-uniform, before any barrier; rows >= Tv of the workspace are not read
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;           // q at +0, k at +H
    float* st = stats + ((long)b * gridDim.x + head) * T;                // this (clip, head)'s rows of plane 0
    const float c2 = scale * LOG2E;

    const int nblk = (Tv + KB - 1) / KB;
    const int qt = blockIdx.z * AML_NW + wv;
    const bool live = qt * 16 < Tv;              // wave-uniform; idle wavefronts still take part in staging and barriers
    const int qrow = qt * 16 + fr, qr = qrow < Tv ? qrow : Tv - 1;
    float4 qf[DG];
#pragma unroll
    for (int G_ = 0; G_ < DG; ++G_) qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);

    float m_run = -INFINITY, l_run = 0.f;
    for (int blk = 0; blk < nblk; ++blk) {
        const int k0 = blk * KB;
        __syncthreads();                         // every wavefront is done with the previous block
        stage_f32<KB, D, AML_NTH>(Ks, base + H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        __syncthreads();
        if (!live) continue;
        f32x4 s[NTB];
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(Ks + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s[kt], kf, qf[G_]);                 // S^T [key][q]
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (k0 + kt * 16 + g * 4 + r < Tv) ? aml_score(s[kt][r], c2) : -INFINITY;       // log2 domain
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);    // finite: every block holds at least one key < Tv
        const float alpha = exp2f(m_run - m_new);             // 0 for the first block (m_run = -inf)
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += exp2f(s[kt][r] - m_new);      // 0 for keys >= Tv
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * alpha + sum;
        m_run = m_new;
    }
    if (live && g == 0 && qrow < Tv) {
        st[qrow] = m_run;
        st[stats_plane + qrow] = 1.f / l_run;
    }
}

// ---------------------------------------------------------------------------------------------- maps: one 128 x 128 tile
// fuse: 0 = this workgroup's one head (blockIdx.x), 1 = mean, 2 = max, 3 = min over heads [0, heads)
template <int D, bool GRAD>
__global__ __launch_bounds__(AML_NTH) void attention_maps_long_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                      const _Float16* __restrict__ dctx, long dctx_lo, float dscale, int fuse,
                                                                      float* __restrict__ out, const float* __restrict__ stats, long stats_plane,
                                                                      const int* __restrict__ frames, int T, int H, int heads, int dm,
                                                                      float scale) {
    constexpr int KB = AML_SB, NTB = KB / 16, PITCH = D + 4, DG = D / 16;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* Ks = smf;
    float* Vs = smf + KB * PITCH;                         // GRAD only
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, nb = (T + AML_RB - 1) / AML_RB;
    const int row0 = ((int)blockIdx.z / nb) * AML_RB, k0 = ((int)blockIdx.z % nb) * KB;
    const int h0 = fuse ? 0 : (int)blockIdx.x, h1 = fuse ? heads : h0 + 1;
    const int Tv = aml_valid_rows(frames, b, T);
    const long ld = 3L * H;
    const float c2 = scale * LOG2E;
    float* obase = out + (fuse ? (long)b : (long)b * heads + h0) * T * T;
    const bool vec = (T & 3) == 0;                        // rows start 16-byte aligned

    if (row0 >= Tv || k0 >= Tv) {                // workgroup-uniform, before any barrier: this tile is zeros
        const int rows = T - row0 < AML_RB ? T - row0 : AML_RB;
        for (int i = tid; i < rows * (KB / 4); i += AML_NTH) {
            float* o = obase + (long)(row0 + i / (KB / 4)) * T + k0 + (i % (KB / 4)) * 4;
            const int key = k0 + (i % (KB / 4)) * 4;
            if (vec) {
                if (key < T) *(float4*)o = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (key + r < T) o[r] = 0.f;
            }
        }
        return;
    }

    const int qrow = row0 + wv * 16 + fr, qr = qrow < Tv ? qrow : Tv - 1;
    const bool live = row0 + wv * 16 < Tv;       // wave-uniform; idle wavefronts stage, meet the barriers and store zeros

    f32x4 acc[NTB];
#pragma unroll
    for (int kt = 0; kt < NTB; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int head = h0; head < h1; ++head) {
        const _Float16* base = qkv + (long)b * T * ld + head * dm;           // q at +0, k at +H, v at +2H
        if (head != h0) __syncthreads();                                      // the previous head's blocks are no longer read
        stage_f32<KB, D, AML_NTH>(Ks, base + H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        if (GRAD) stage_f32<KB, D, AML_NTH>(Vs, base + 2 * H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        __syncthreads();
        if (!live) continue;

        const float* st = stats + ((long)b * heads + head) * T;
        const float m = st[qr], inv = st[stats_plane + qr];
        float4 qf[DG], of[GRAD ? DG : 1];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
        if (GRAD) {
            const _Float16* dob = dctx + (long)b * T * H + head * dm;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) of[G_] = grow4(dob, dctx_lo, (long)qr * H, 16 * G_ + 4 * g, dm);
        }
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(Ks + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s, kf, qf[G_]);                     // S^T  [key][q]
                if (GRAD) {
                    const float4 vf = *(const float4*)(Vs + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                    MFMA4(dp, vf, of[G_]);                // dP^T [key][q]
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = 0.f;                            // keys >= Tv
                if (k0 + kt * 16 + g * 4 + r < Tv) {
                    v = exp2f(aml_exponent(s[r], c2, m)) * inv;
                    if (GRAD) {
                        v = v * (dp[r] * dscale);
                        v = v < 0.f ? 0.f : v;            // (P * dP)^+; a NaN stays a NaN
                    }
                }
                // fold this head into the fused tile, heads in index order (a NaN wins max and min as it wins the sum)
                const float a = acc[kt][r];
                if (head == h0) acc[kt][r] = v;
                else if (fuse == 1) acc[kt][r] = a + v;
                else if (fuse == 2) acc[kt][r] = (v > a || v != v) ? v : a;
                else acc[kt][r] = (v < a || v != v) ? v : a;
            }
        }
    }
    if (qrow >= T) return;

    const float mean = qrow < Tv ? (fuse == 1 ? 1.f / (float)heads : 1.f) : 0.f;     // rows Tv <= q < T: zeros (idle wavefronts hold zeros)
    float* orow = obase + (long)qrow * T;
#pragma unroll
    for (int kt = 0; kt < NTB; ++kt) {
        const int key = k0 + kt * 16 + g * 4;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = qrow < Tv ? acc[kt][r] * mean : 0.f;
        if (vec) {
            if (key < T) *(float4*)(orow + key) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key + r < T) orow[key + r] = v[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------- value: dV = P^T dO, dQ = dK = 0
template <int D>
__global__ __launch_bounds__(AML_NTH) void attention_bwd_value_long_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                           const _Float16* __restrict__ dctx, long dctx_lo,
                                                                           _Float16* __restrict__ dqkv, long dqkv_lo,
                                                                           const float* __restrict__ stats, long stats_plane,
                                                                           const int* __restrict__ frames, int T, int H, int dm, float scale) {
    constexpr int SQB = AML_SB, NQT = SQB / 16, PITCH = D + 4, DG = D / 16;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* Qs = smf;
    float* Os = smf + SQB * PITCH;
    float* rmax = smf + 2 * SQB * PITCH;
    float* rinv = rmax + SQB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * AML_RB;
    const int Tv = aml_valid_rows(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    const _Float16* dob = dctx + (long)b * T * H + head * dm;
    _Float16* dbase = dqkv + (long)b * T * ld + head * dm;
    const float* st = stats + ((long)b * gridDim.x + head) * T;
    const float c2 = scale * LOG2E;

    // this block's rows: the Q and K thirds are zeros everywhere, the V third from Tv on
    const int r1 = T < row0 + AML_RB ? T : row0 + AML_RB;
    aml_zero_rows(dbase, dqkv_lo, ld, 0, row0, r1, dm, tid);
    aml_zero_rows(dbase, dqkv_lo, ld, H, row0, r1, dm, tid);
    if (Tv < r1) aml_zero_rows(dbase, dqkv_lo, ld, 2 * H, Tv > row0 ? Tv : row0, r1, dm, tid);
    if (row0 >= Tv) return;                      // workgroup-uniform, before any barrier

    const int nblk = (Tv + SQB - 1) / SQB;
    const int kt = blockIdx.z * AML_NW + wv;
    const bool live = kt * 16 < Tv;
    const int krow = kt * 16 + fr, kr_ = krow < Tv ? krow : Tv - 1;
    float4 kf[DG];
#pragma unroll
    for (int G_ = 0; G_ < DG; ++G_) kf[G_] = grow4(base + H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
    f32x4 dvt[DG];
#pragma unroll
    for (int dt = 0; dt < DG; ++dt) dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int blk = 0; blk < nblk; ++blk) {       // query blocks in index order
        const int q0 = blk * SQB;
        __syncthreads();
        stage_f32<SQB, D, AML_NTH>(Qs, base + (long)q0 * ld, qkv_lo, ld, Tv - q0, dm, tid);
        stage_f32<SQB, D, AML_NTH>(Os, dob + (long)q0 * H, dctx_lo, (long)H, Tv - q0, dm, tid);
        if (tid < SQB) {
            const bool in = q0 + tid < Tv;       // rows >= Tv of the workspace are not read
            rmax[tid] = in ? st[q0 + tid] : 0.f;
            rinv[tid] = in ? st[stats_plane + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        for (int qt = 0; qt < NQT && q0 + qt * 16 < Tv; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 qa = *(const float4*)(Qs + (qt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s, qa, kf[G_]);                     // S [q][key]
            }
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qt * 16 + g * 4 + r;        // this lane's query rows of the block; its key column = krow
                p[r] = 0.f;
                if (q0 + q < Tv && krow < Tv) p[r] = exp2f(aml_exponent(s[r], c2, rmax[q])) * rinv[q];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* orw = Os + (qt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt)
                    dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(orw[16 * dt], p[r], dvt[dt], 0, 0, 0);       // dV^T [d][key]
            }
        }
    }
    if (live && krow < Tv) {
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) {
            if (dt * 16 + g * 4 >= dm) continue;
            const float vv[4] = {dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]};
            store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);          // checked split conversion
        }
    }
}

// ---------------------------------------------------------------------------------------------- rollout
// rollout_step_kernel of attention_maps.hip (16 rows x 64 columns per workgroup, contraction in chunks of 64, the row sums on a
// fifth accumulator) with T the stride and Tv every bound: the chunks, and so the summation order, depend on Tv alone.  Y is
// written for every i, j < T: zeros outside the Tv x Tv block.
constexpr int ROL_KC = 64, ROL_NC = 64, ROL_PITCH = 68;

__global__ __launch_bounds__(256) void rollout_step_long_kernel(const float* __restrict__ M, const float* __restrict__ X, float* __restrict__ Y,
                                                                float alpha, float beta, float gamma, int normalize,
                                                                const int* __restrict__ frames, int T) {
    __shared__ float Ms[16 * ROL_PITCH];
    __shared__ float Xs[ROL_KC * ROL_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.x * ROL_NC, i0 = blockIdx.y * 16;
    const int Tv = aml_valid_rows(frames, blockIdx.z, T);
    const long mat = (long)blockIdx.z * T * T;
    const float* Mb = M + mat;
    const float* Xb = X + mat;

    if (i0 >= Tv || j0 >= Tv) {                  // workgroup-uniform, before any barrier
        for (int i = tid; i < 16 * ROL_NC; i += 256) {
            const int r = i / ROL_NC, c = i % ROL_NC;
            if (i0 + r < T && j0 + c < T) Y[mat + (long)(i0 + r) * T + j0 + c] = 0.f;
        }
        return;
    }

    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, rs = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Tv; k0 += ROL_KC) {
        if (k0) __syncthreads();
        for (int i = tid; i < 16 * ROL_KC; i += 256) {
            const int r = i / ROL_KC, c = i % ROL_KC;
            Ms[r * ROL_PITCH + c] = (i0 + r < Tv && k0 + c < Tv) ? Mb[(long)(i0 + r) * T + k0 + c] : 0.f;
        }
        for (int i = tid; i < ROL_KC * ROL_NC; i += 256) {
            const int r = i / ROL_NC, c = i % ROL_NC;
            Xs[r * ROL_PITCH + c] = (k0 + r < Tv && j0 + c < Tv) ? Xb[(long)(k0 + r) * T + j0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ROL_KC; k += 4) {
            const float a = Ms[fr * ROL_PITCH + k + g];                      // A[i = fr][k + g]
            const float x = Xs[(k + g) * ROL_PITCH + wv * 16 + fr];          // B[k + g][j = fr]
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x, acc, 0, 0, 0);
            rs = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.f, rs, 0, 0, 0);
        }
    }
    const int j = j0 + wv * 16 + fr;
    if (j >= T) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * g + r;
        if (i >= T) continue;
        const long o = (long)i * T + j;
        if (i >= Tv || j >= Tv) {
            Y[mat + o] = 0.f;
            continue;
        }
        const float num = alpha * Xb[o] + beta * acc[r] + gamma * Mb[o];
        Y[mat + o] = normalize ? num / (alpha + beta * rs[r]) : num;
    }
}

// rel[b][j] = (1/Tv) sum_{i < Tv} X[b][i][j] for j < Tv, 0 for Tv <= j < T: one thread per column, rows in order
__global__ __launch_bounds__(256) void rollout_relevance_long_kernel(const float* __restrict__ X, float* __restrict__ rel,
                                                                     const int* __restrict__ frames, int T) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= T) return;
    const int Tv = aml_valid_rows(frames, b, T);
    if (j >= Tv) {
        rel[(long)b * T + j] = 0.f;
        return;
    }
    const float* Xb = X + (long)b * T * T;
    float s = 0.f;
    for (int i = 0; i < Tv; ++i) s += Xb[(long)i * T + j];
    rel[(long)b * T + j] = s / (float)Tv;
}

template <int D>
static int launch_stats_long(const _Float16* qkv, long ql, float* ws, const int* fv, int B, int T, int H, int heads, int dm, float scale,
                             hipStream_t s) {
    constexpr int ls = aml_lds_stats(D);
    if (ls > 64 * 1024 && advh_ensure_lds((const void*)attention_stats_long_kernel<D>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((attention_stats_long_kernel<D>), dim3(heads, B, (T + AML_RB - 1) / AML_RB), dim3(AML_NTH), ls, s, qkv, ql, ws,
                       (long)B * heads * T, fv, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

template <int D, bool GRAD>
static int launch_maps_long(const _Float16* qkv, long ql, const _Float16* dctx, long dl, float dscale, int fuse, float* out, float* ws,
                            const int* fv, int B, int T, int H, int heads, int dm, hipStream_t s) {
    constexpr int lm = aml_lds_maps(D, GRAD);
    static_assert(lm <= 160 * 1024 && aml_lds_stats(D) <= 160 * 1024, "the staged blocks must fit");
    if (lm > 64 * 1024 && advh_ensure_lds((const void*)attention_maps_long_kernel<D, GRAD>) != ADVH_OK) return ADVH_ELAUNCH;
    const float scale = 1.f / sqrtf((float)dm);
    const int rc = launch_stats_long<D>(qkv, ql, ws, fv, B, T, H, heads, dm, scale, s);
    if (rc != ADVH_OK) return rc;
    const int nb = (T + AML_RB - 1) / AML_RB;
    hipLaunchKernelGGL((attention_maps_long_kernel<D, GRAD>), dim3(fuse ? 1 : heads, B, nb * nb), dim3(AML_NTH), lm, s, qkv, ql, dctx, dl,
                       dscale, fuse, out, (const float*)ws, (long)B * heads * T, fv, T, H, heads, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

template <int D>
static int launch_value_long(const _Float16* qkv, long ql, const _Float16* dctx, long dl, _Float16* dqkv, long ol, float* ws, const int* fv,
                             int B, int T, int H, int heads, int dm, hipStream_t s) {
    constexpr int lv = aml_lds_value(D);
    static_assert(lv <= 160 * 1024, "both staged matrices must fit");
    if (lv > 64 * 1024 && advh_ensure_lds((const void*)attention_bwd_value_long_kernel<D>) != ADVH_OK) return ADVH_ELAUNCH;
    const float scale = 1.f / sqrtf((float)dm);
    const int rc = launch_stats_long<D>(qkv, ql, ws, fv, B, T, H, heads, dm, scale, s);
    if (rc != ADVH_OK) return rc;
    hipLaunchKernelGGL((attention_bwd_value_long_kernel<D>), dim3(heads, B, (T + AML_RB - 1) / AML_RB), dim3(AML_NTH), lv, s, qkv, ql, dctx,
                       dl, dqkv, ol, (const float*)ws, (long)B * heads * T, fv, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

}  // namespace advh

using namespace advh;

extern "C" int advh_attention_maps_long(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, float dscale, int fuse, float* out,
                                        float* ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !out || !ws || B <= 0 || T <= 0 || heads <= 0 || H <= 0 || H % heads) return ADVH_EINVAL;
    if (fuse < 0 || fuse > 3 || !isfinite(dscale)) return ADVH_EINVAL;
    if (qkv_lo < 0 || qkv_lo % 8) return ADVH_EINVAL;
    if (dctx && (qkv_lo ? (dctx_lo <= 0 || dctx_lo % 8) : dctx_lo != 0)) return ADVH_EINVAL;     // both split or both plain fp16
    const int dm = H / heads;
    const long nb = ((long)T + AML_RB - 1) / AML_RB;
    if (dm % 8 || dm > 128 || B > 65535 || nb * nb > 65535) return ADVH_EUNSUPPORTED;            // the grid's y and z extents
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    const _Float16* d = (const _Float16*)dctx;
    const long dl = dctx ? (long)dctx_lo : 0;
    const int* fv = (const int*)frames;
#define AML(D_)                                                                                                             \
    return dctx ? launch_maps_long<D_, true>(q, (long)qkv_lo, d, dl, dscale, fuse, out, ws, fv, B, T, H, heads, dm, s)     \
                : launch_maps_long<D_, false>(q, (long)qkv_lo, d, dl, dscale, fuse, out, ws, fv, B, T, H, heads, dm, s)
    if (dm <= 32) AML(32);
    if (dm <= 64) AML(64);
    AML(128);
#undef AML
}

extern "C" int advh_attention_bwd_value_long(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                             float* ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || !ws || B <= 0 || T <= 0 || heads <= 0 || H <= 0 || H % heads) return ADVH_EINVAL;
    if (qkv_lo < 0 || qkv_lo % 8) return ADVH_EINVAL;
    if (qkv_lo ? (dctx_lo <= 0 || dctx_lo % 8 || dqkv_lo <= 0 || dqkv_lo % 8) : (dctx_lo != 0 || dqkv_lo != 0)) return ADVH_EINVAL;   // all split or all fp16
    const int dm = H / heads;
    const long nb = ((long)T + AML_RB - 1) / AML_RB;
    if (dm % 8 || dm > 128 || B > 65535 || nb > 65535) return ADVH_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    const _Float16* d = (const _Float16*)dctx;
    _Float16* o = (_Float16*)dqkv;
    const int* fv = (const int*)frames;
    if (dm <= 32) return launch_value_long<32>(q, (long)qkv_lo, d, (long)dctx_lo, o, (long)dqkv_lo, ws, fv, B, T, H, heads, dm, s);
    if (dm <= 64) return launch_value_long<64>(q, (long)qkv_lo, d, (long)dctx_lo, o, (long)dqkv_lo, ws, fv, B, T, H, heads, dm, s);
    return launch_value_long<128>(q, (long)qkv_lo, d, (long)dctx_lo, o, (long)dqkv_lo, ws, fv, B, T, H, heads, dm, s);
}

extern "C" int advh_rollout_step_long(const float* M, const float* X, float* Y, float alpha, float beta, float gamma, int normalize,
                                      const int32_t* frames, int B, int T, advh_stream_t stream) {
    if (!M || !X || !Y || Y == X || Y == M || B <= 0 || T <= 0) return ADVH_EINVAL;
    if (B > 65535 || ((long)T + 15) / 16 > 65535) return ADVH_EUNSUPPORTED;
    hipLaunchKernelGGL(rollout_step_long_kernel, dim3((T + ROL_NC - 1) / ROL_NC, (T + 15) / 16, B), dim3(256), 0, (hipStream_t)stream, M, X, Y,
                       alpha, beta, gamma, normalize, (const int*)frames, T);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_rollout_relevance_long(const float* X, float* rel, const int32_t* frames, int B, int T, advh_stream_t stream) {
    if (!X || !rel || B <= 0 || T <= 0) return ADVH_EINVAL;
    if (B > 65535 || ((long)T + 15) / 16 > 65535) return ADVH_EUNSUPPORTED;
    hipLaunchKernelGGL(rollout_relevance_long_kernel, dim3((T + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, X, rel, (const int*)frames, T);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention_maps_long)
