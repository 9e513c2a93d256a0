// Attention backward for clips of any length: dqkv from (qkv, dctx) for softmax(Q K^T / sqrt(d)) V, any T >= 1, head dim <= 128.
//
// The whole-clip kernels (backward.hip, attention_bwd_x3.hip, attention_bwd_f32.hip, batch and ragged instances) hold a (clip, head)
// in LDS and stop at T = 256 frames.  Here two kernels run one after the other on the same stream, each streaming the other side's
// rows through LDS in blocks of 128, with the row statistics of the softmax in a caller-provided fp32 workspace between them; no
// atomics.  Every product runs on v_mfma_f32_16x16x4_f32 for both operand formats: split plane pairs and plain fp16 (lo == 0) are
// joined to fp32 when staged (attention_f32_tiles.h); the operand layouts are those described at the top of attention_bwd_f32.hip.
//
//   query kernel, grid (heads, B, ceil(T / QB)), QB = 128: a workgroup owns one block of eight 16-query tiles, one per wavefront
//     (q and dO fragments in registers), and streams K and V in key blocks of KB = 128 rows, twice:
//       sweep 1  S^T, dP^T per block; running maximum m (log2 domain), running sum l and running sum_j e^(s_j - m) dP_j, the two sums
//                rescaled by alpha = 2^(m_old - m_new) when a block raises the maximum; at the end delta = that / l, and
//                (m, 1 / l, delta) go to stats[3][B * heads * T]
//       sweep 2  S^T, dP^T again; dS^T = P (dP - delta) scale in registers, which are the B operand of dQ^T += K^T dS^T (pass A of
//                attention_bwd_f32.hip); stores the Q third
//   key kernel, grid (heads, B, ceil(T / KWB)), KWB = 128: a workgroup owns one block of eight 16-key tiles; the k and v fragments
//     and the dK^T / dV^T accumulators stay in registers (pass B there).  It streams Q and dO in query blocks of SQB = 128 rows, in
//     index order, with those rows' (m, 1 / l, delta); per block S, dP, P = exp2(s c2 - m) / l, dS, dK^T += Q^T dS, dV^T += dO^T P.
//     Both staged matrices fit at every head dim, so there is no B2 sub-pass.
// Nine products per (query, key) pair; the whole-clip kernel makes seven.
//
// S and dP are formed three times.  Each time visits d in the order of MFMA4 (G_, then x, y, z, w) on the same joined operand
// values, and a * b commutes, so the three are bit-equal (the fp32 MFMA is a k-ordered fmaf chain); the scaled score is one rounded
// product (bwl_score / bwl_exponent: no contraction into the subtraction of m) everywhere.  dS_ii = P_ii (dP_ii - delta_i) of a
// peaked row depends on it (attention_bwd_x3.hip, MFMA_X3_SWAPPED), and so does every row sum of dS.
//
// Per-clip bound: frames == nullptr -> Tv = T; otherwise Tv = clamp(frames[b], 1, T), the semantics of attention_long.hip.  T stays
// the row STRIDE; every bound a stage sees is Tv.  Rows Tv <= t < T of dqkv are zeros in every plane: the query kernel zeroes the Q
// third of its own block, the key kernel the K and V thirds of its own.  Rows >= Tv of qkv / dctx / stats are never read.  A
// workgroup whose block lies at or beyond Tv returns after zeroing, before any barrier.  Blocks are aligned to row 0, so what is
// computed for a clip depends on Tv alone.
//
//   instance (each kernel)   dynamic LDS: two fp32 matrices [128][D + 4]  (+ 3 x 128 floats of statistics in the key kernel)
//   D =  32                   36 864 B |  38 400 B
//   D =  64                   69 632 B |  71 168 B
//   D = 128                  135 168 B | 136 704 B
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"
#include "attention_f32_tiles.h"

namespace advh {

constexpr int BWL_NW = 8;                          // wavefronts per workgroup: two per SIMD
constexpr int BWL_QB = 16 * BWL_NW;                // queries per query-kernel workgroup
constexpr int BWL_KB = 128;                        // staged key block of the query kernel
constexpr int BWL_KWB = 16 * BWL_NW;               // keys per key-kernel workgroup
constexpr int BWL_SQB = 128;                       // staged query block of the key kernel

constexpr int bwl_lds_query(int D) { return 2 * BWL_KB * (D + 4) * 4; }
constexpr int bwl_lds_key(int D) { return (2 * BWL_SQB * (D + 4) + 3 * BWL_SQB) * 4; }

typedef _Float16 bwl_h4 __attribute__((ext_vector_type(4)));

// The score in the log2 domain and the exponent of a probability, with the product ROUNDED before m is subtracted, at every site:
// contraction is off here, or the compiler fuses `s * c2 - m` into one fma where the product is not needed on its own (sweep 2, the
// key kernel) and not where it is (sweep 1, which takes the maximum of the products).  The three evaluations of P then differ by
// |s c2| 2^-24 and the rows of dS stop summing to zero: the ordered input of the tests measured dq at 7.4e-6 of its maximum.
__device__ __forceinline__ float bwl_score(float s, float c2) {
#pragma clang fp contract(off)
    return s * c2;
}
__device__ __forceinline__ float bwl_exponent(float s, float c2, float m) {
#pragma clang fp contract(off)
    const float t = s * c2;
    return t - m;
}

__device__ __forceinline__ int bwl_valid_rows(const int* frames, int b, int T) {
    if (!frames) return T;
    const int f = frames[b];
    return f < 1 ? 1 : (f > T ? T : f);
}

// rows max(Tv, row0) <= t < min(T, row0 + rows) of `thirds` thirds of dqkv from column `col0` on (this head's dm columns) <- 0 in
// every plane; dm % 8 == 0: 8-byte stores
__device__ __forceinline__ void bwl_zero_rows(_Float16* dbase, long dqkv_lo, long ld, int H, int col0, int thirds, int row0, int rows, int Tv,
                                              int T, int dm, int tid, int nth) {
    const int z0 = Tv > row0 ? Tv : row0, z1 = T < row0 + rows ? T : row0 + rows, c4 = dm / 4, n = (z1 - z0) * c4;
    for (int i = tid; i < n; i += nth) {
        const long o = (long)(z0 + i / c4) * ld + col0 + (i % c4) * 4;
        for (int t = 0; t < thirds; ++t) {
            *(bwl_h4*)(dbase + o + (long)t * H) = bwl_h4{0, 0, 0, 0};
            if (dqkv_lo) *(bwl_h4*)(dbase + dqkv_lo + o + (long)t * H) = bwl_h4{0, 0, 0, 0};
        }
    }
}

template <int D>
__global__ __launch_bounds__(64 * BWL_NW) void attention_bwd_long_query_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                               const _Float16* __restrict__ dctx, long dctx_lo,
                                                                               _Float16* __restrict__ dqkv, long dqkv_lo, float* __restrict__ stats,
                                                                               long stats_plane, const int* __restrict__ frames, int T, int H,
                                                                               int dm, float scale) {
    constexpr int KB = BWL_KB, NTB = KB / 16, PITCH = D + 4, DG = D / 16, NTH = 64 * BWL_NW;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* Ks = smf;
    float* Vs = smf + KB * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * BWL_QB;
    const int Tv = bwl_valid_rows(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;           // q at +0, k at +H, v at +2H
    const _Float16* dob = dctx + (long)b * T * H + head * dm;
    _Float16* dbase = dqkv + (long)b * T * ld + head * dm;
    float* st = stats + ((long)b * gridDim.x + head) * T;                // this (clip, head)'s rows of plane 0
    const float c2 = scale * LOG2E;

    bwl_zero_rows(dbase, dqkv_lo, ld, H, 0, 1, row0, BWL_QB, Tv, T, dm, tid, NTH);
    if (row0 >= Tv) return;                      // workgroup-uniform, before any barrier

    const int nblk = (Tv + KB - 1) / KB;
    const int qt = blockIdx.z * BWL_NW + wv;
    const bool live = qt * 16 < Tv;              // wave-uniform; idle wavefronts still take part in staging and barriers
    const int qrow = qt * 16 + fr, qr = qrow < Tv ? qrow : Tv - 1;
    float4 qf[DG], of[DG];
#pragma unroll
    for (int G_ = 0; G_ < DG; ++G_) {
        qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
        of[G_] = grow4(dob, dctx_lo, (long)qr * H, 16 * G_ + 4 * g, dm);
    }

    // ------------------------------------------------------------------ sweep 1: m, l, sum e^(s - m) dP
    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
    for (int blk = 0; blk < nblk; ++blk) {
        const int k0 = blk * KB;
        __syncthreads();                         // every wavefront is done with the previous block
        stage_f32<KB, D, NTH>(Ks, base + H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        stage_f32<KB, D, NTH>(Vs, base + 2 * H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        __syncthreads();
        if (!live) continue;
        f32x4 s[NTB], dp[NTB];
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(Ks + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                const float4 vf = *(const float4*)(Vs + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s[kt], kf, qf[G_]);                 // S^T  [key][q]
                MFMA4(dp[kt], vf, of[G_]);                // dP^T [key][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (k0 + kt * 16 + g * 4 + r < Tv) ? bwl_score(s[kt][r], c2) : -INFINITY;       // log2 domain
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);    // finite: every block holds at least one key < Tv
        const float alpha = exp2f(m_run - m_new);             // 0 for the first block (m_run = -inf)
        float sum = 0.f, acc = 0.f;
#pragma unroll
        for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = exp2f(s[kt][r] - m_new);      // 0 for keys >= Tv
                sum += e;
                acc += e * dp[kt][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        l_run = l_run * alpha + sum;
        d_run = d_run * alpha + acc;
        m_run = m_new;
    }
    const float inv = 1.f / l_run, del = d_run * inv;
    if (live && g == 0 && qrow < Tv) {
        st[qrow] = m_run;
        st[stats_plane + qrow] = inv;
        st[2 * stats_plane + qrow] = del;
    }

    // ------------------------------------------------------------------ sweep 2: dQ^T += K^T dS^T
    f32x4 o[DG];
#pragma unroll
    for (int dt = 0; dt < DG; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int blk = 0; blk < nblk; ++blk) {
        const int k0 = blk * KB;
        __syncthreads();
        stage_f32<KB, D, NTH>(Ks, base + H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        stage_f32<KB, D, NTH>(Vs, base + 2 * H + (long)k0 * ld, qkv_lo, ld, Tv - k0, dm, tid);
        __syncthreads();
        if (!live) continue;
#pragma unroll 1                                             // nothing is indexed by kt but LDS rows: one tile's registers at a time
        for (int kt = 0; kt < NTB && k0 + kt * 16 < Tv; ++kt) {          // tiles past Tv hold dS = 0
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(Ks + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                const float4 vf = *(const float4*)(Vs + (kt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s, kf, qf[G_]);
                MFMA4(dp, vf, of[G_]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float ds = 0.f;                               // keys >= Tv: p = 0
                if (k0 + kt * 16 + g * 4 + r < Tv) {
                    const float p = exp2f(bwl_exponent(s[r], c2, m_run)) * inv;
                    ds = p * (dp[r] - del) * scale;           // dS^T [key][q]
                }
                const float* kr = Ks + (kt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[16 * dt], ds, o[dt], 0, 0, 0);        // dQ^T [d][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (live && qrow < Tv) {
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) {
            if (dt * 16 + g * 4 >= dm) continue;
            const float v[4] = {o[dt][0], o[dt][1], o[dt][2], o[dt][3]};
            store_h_rt<4>(dbase, (long)qrow * ld + dt * 16 + g * 4, dqkv_lo, v);
        }
    }
}

template <int D>
__global__ __launch_bounds__(64 * BWL_NW) void attention_bwd_long_key_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                             const _Float16* __restrict__ dctx, long dctx_lo,
                                                                             _Float16* __restrict__ dqkv, long dqkv_lo,
                                                                             const float* __restrict__ stats, long stats_plane,
                                                                             const int* __restrict__ frames, int T, int H, int dm, float scale) {
    constexpr int SQB = BWL_SQB, NQT = SQB / 16, PITCH = D + 4, DG = D / 16, NTH = 64 * BWL_NW;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* Qs = smf;
    float* Os = smf + SQB * PITCH;
    float* rmax = smf + 2 * SQB * PITCH;
    float* rinv = rmax + SQB;
    float* rdel = rinv + SQB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * BWL_KWB;
    const int Tv = bwl_valid_rows(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    const _Float16* dob = dctx + (long)b * T * H + head * dm;
    _Float16* dbase = dqkv + (long)b * T * ld + head * dm;
    const float* st = stats + ((long)b * gridDim.x + head) * T;
    const float c2 = scale * LOG2E;

    bwl_zero_rows(dbase, dqkv_lo, ld, H, H, 2, row0, BWL_KWB, Tv, T, dm, tid, NTH);
    if (row0 >= Tv) return;                      // workgroup-uniform, before any barrier

    const int nblk = (Tv + SQB - 1) / SQB;
    const int kt = blockIdx.z * BWL_NW + wv;
    const bool live = kt * 16 < Tv;
    const int krow = kt * 16 + fr, kr_ = krow < Tv ? krow : Tv - 1;
    float4 kf[DG], vf[DG];
#pragma unroll
    for (int G_ = 0; G_ < DG; ++G_) {
        kf[G_] = grow4(base + H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
        vf[G_] = grow4(base + 2 * H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
    }
    f32x4 dkt[DG], dvt[DG];
#pragma unroll
    for (int dt = 0; dt < DG; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int blk = 0; blk < nblk; ++blk) {       // query blocks in index order
        const int q0 = blk * SQB;
        __syncthreads();
        stage_f32<SQB, D, NTH>(Qs, base + (long)q0 * ld, qkv_lo, ld, Tv - q0, dm, tid);
        stage_f32<SQB, D, NTH>(Os, dob + (long)q0 * H, dctx_lo, (long)H, Tv - q0, dm, tid);
        if (tid < SQB) {
            const bool in = q0 + tid < Tv;       // rows >= Tv of the workspace are not read
            rmax[tid] = in ? st[q0 + tid] : 0.f;
            rinv[tid] = in ? st[stats_plane + q0 + tid] : 0.f;
            rdel[tid] = in ? st[2 * stats_plane + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        for (int qt = 0; qt < NQT && q0 + qt * 16 < Tv; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 qa = *(const float4*)(Qs + (qt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                const float4 oa = *(const float4*)(Os + (qt * 16 + fr) * PITCH + 16 * G_ + 4 * g);
                MFMA4(s, qa, kf[G_]);                     // S  [q][key]
                MFMA4(dp, oa, vf[G_]);                    // dP [q][key]
            }
            float p[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qt * 16 + g * 4 + r;        // this lane's query rows of the block; its key column = krow
                p[r] = 0.f;
                ds[r] = 0.f;
                if (q0 + q < Tv && krow < Tv) {
                    p[r] = exp2f(bwl_exponent(s[r], c2, rmax[q])) * rinv[q];
                    ds[r] = p[r] * (dp[r] - rdel[q]) * scale;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* qrw = Qs + (qt * 16 + 4 * g + r) * PITCH + fr;
                const float* orw = Os + (qt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt) {
                    dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qrw[16 * dt], ds[r], dkt[dt], 0, 0, 0);      // dK^T [d][key]
                    dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(orw[16 * dt], p[r], dvt[dt], 0, 0, 0);       // dV^T [d][key]
                }
            }
        }
    }
    if (live && krow < Tv) {
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) {
            if (dt * 16 + g * 4 >= dm) continue;
            const float kv[4] = {dkt[dt][0], dkt[dt][1], dkt[dt][2], dkt[dt][3]};
            store_h_rt<4>(dbase, (long)krow * ld + H + dt * 16 + g * 4, dqkv_lo, kv);
            const float vv[4] = {dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]};
            store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);
        }
    }
}

template <int D>
static int launch_bwd_long(const _Float16* qkv, long ql, const _Float16* dctx, long dl, _Float16* dqkv, long ol, float* stats, const int* fv,
                           int B, int T, int H, int heads, int dm, hipStream_t s) {
    constexpr int lq = bwl_lds_query(D), lk = bwl_lds_key(D);
    static_assert(lq <= 160 * 1024 && lk <= 160 * 1024, "both staged matrices must fit");
    if (lq > 64 * 1024 && advh_ensure_lds((const void*)attention_bwd_long_query_kernel<D>) != ADVH_OK) return ADVH_ELAUNCH;
    if (lk > 64 * 1024 && advh_ensure_lds((const void*)attention_bwd_long_key_kernel<D>) != ADVH_OK) return ADVH_ELAUNCH;
    const float scale = 1.f / sqrtf((float)dm);
    const long plane = (long)B * heads * T;
    hipLaunchKernelGGL((attention_bwd_long_query_kernel<D>), dim3(heads, B, (T + BWL_QB - 1) / BWL_QB), dim3(64 * BWL_NW), lq, s, qkv, ql, dctx,
                       dl, dqkv, ol, stats, plane, fv, T, H, dm, scale);
    hipLaunchKernelGGL((attention_bwd_long_key_kernel<D>), dim3(heads, B, (T + BWL_KWB - 1) / BWL_KWB), dim3(64 * BWL_NW), lk, s, qkv, ql, dctx,
                       dl, dqkv, ol, (const float*)stats, plane, fv, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

}  // namespace advh

using namespace advh;

// The limits both entries share, decided before any launch: head dim, and the grid's y and z extents.
static int bwd_long_unsupported(int B, int T, int dm) {
    const long nb = ((long)T + BWL_QB - 1) / BWL_QB;
    return dm % 8 || dm > 128 || B > 65535 || nb > 65535;
}

static int bwd_long(const void* qkv, long ql, const void* dctx, long dl, void* dqkv, long ol, float* stats, const int32_t* frames, int B, int T,
                    int H, int heads, advh_stream_t stream) {
    const int dm = H / heads;
    if (bwd_long_unsupported(B, T, dm)) return ADVH_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    const _Float16* d = (const _Float16*)dctx;
    _Float16* o = (_Float16*)dqkv;
    const int* fv = (const int*)frames;
    if (dm <= 32) return launch_bwd_long<32>(q, ql, d, dl, o, ol, stats, fv, B, T, H, heads, dm, s);
    if (dm <= 64) return launch_bwd_long<64>(q, ql, d, dl, o, ol, stats, fv, B, T, H, heads, dm, s);
    return launch_bwd_long<128>(q, ql, d, dl, o, ol, stats, fv, B, T, H, heads, dm, s);
}

extern "C" size_t advh_attention_bwd_long_ws_bytes(int B, int T, int heads) {
    if (B <= 0 || T <= 0 || heads <= 0) return 0;
    const size_t n = (size_t)3 * B * heads * T * sizeof(float);
    return (n + 255) / 256 * 256;
}

extern "C" int advh_attention_bwd_long_f16(const void* qkv, const void* dctx, void* dqkv, float* stats_ws, const int32_t* frames, int B, int T,
                                           int H, int heads, advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || !stats_ws || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    return bwd_long(qkv, 0, dctx, 0, dqkv, 0, stats_ws, frames, B, T, H, heads, stream);
}

extern "C" int advh_attention_bwd_long_split(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                             float* stats_ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || !stats_ws || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    if (qkv_lo <= 0 || dctx_lo <= 0 || dqkv_lo <= 0 || qkv_lo % 8 || dctx_lo % 8 || dqkv_lo % 8) return ADVH_EINVAL;
    return bwd_long(qkv, (long)qkv_lo, dctx, (long)dctx_lo, dqkv, (long)dqkv_lo, stats_ws, frames, B, T, H, heads, stream);
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention_bwd_long)
