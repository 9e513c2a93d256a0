// Attention maps and rollout: the T x T probabilities of one encoder layer, which the flash-style attention kernels keep in
// registers and never write, recomputed from the layer's saved qkv -- and, with the gradient at the attention context, the
// gradient-weighted map of Chefer et al. 2021 -- plus the T x T products of attention rollout (Abnar & Zuidema 2020).
//
//   advh_attention_maps   : P = softmax(Q K^T / sqrt(d))  or  max(P * (dO V^T * dscale), 0), per head or fused over heads
//   advh_rollout_step     : Y = (alpha X + beta M X + gamma M) / (normalize ? alpha + beta rowsum(M) : 1)
//   advh_rollout_relevance: column mean of X
//
// The maps kernel is pass A of attention_bwd_f32.hip without its third product: a wavefront owns one 16-query tile and holds the
// scores TRANSPOSED, s[kt][r] = S[q = l % 16][key = 16 kt + 4 (l / 16) + r], so a query's whole row lives in one lane column (row
// max and sum are two xor-shuffles) and a lane's four registers of a tile are four CONSECUTIVE keys of one output row.  Both
// products (K Q^T and V dO^T, contraction over d) run on v_mfma_f32_16x16x4_f32 with the operands joined to fp32 when staged
// (stage_f32 / grow4 below, as in attention_bwd_f32.hip), for the split format and for plain fp16 alike (qkv_lo == 0).
// One workgroup = (clip, four query tiles, head range): fuse == 0 gives every head its own workgroup; the fused modes loop over
// all heads inside the workgroup, restage K (and V) per head and keep the fused tile in registers -- heads are folded in index
// order, so the result has one summation order, needs no atomics and no [B, heads, T, T] intermediate.
// LDS holds K as fp32 [NKEY][D + 4] and, when two matrices fit (head dim <= 64), V as well; otherwise V's row operands come
// straight from global memory (the one-matrix form of the fp32 backward).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"
#include "attention_f32_tiles.h"

namespace advh {

template <int NT, int D, bool GRAD>
struct AttMaps {
    static constexpr int NW = 4;                                                     // wavefronts = query tiles per workgroup
    static constexpr int NKEY = NT * 16, PITCH = D + 4, DG = D / 16;
    static constexpr int MAT = NKEY * PITCH;                                         // floats of one staged matrix
    static constexpr bool TWO = GRAD && 2 * MAT * 4 <= 160 * 1024;
    static constexpr int LDS_BYTES = (TWO ? 2 : 1) * MAT * 4;
};

// fuse: 0 = this workgroup's one head (blockIdx.y), 1 = mean, 2 = max, 3 = min over heads [0, heads)
template <int NT, int D, bool GRAD>
__global__ __launch_bounds__(256) void attention_maps_kernel(const _Float16* __restrict__ qkv, long qkv_lo, const _Float16* __restrict__ dctx,
                                                             long dctx_lo, float dscale, int fuse, float* __restrict__ out, int T, int H,
                                                             int heads, int dm, float scale) {
    typedef AttMaps<NT, D, GRAD> G;
    constexpr int NKEY = G::NKEY, PITCH = G::PITCH, DG = G::DG, NW = G::NW;
    constexpr bool TWO = G::TWO;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* M0 = smf;                                      // K
    float* M1 = smf + G::MAT;                             // TWO: V

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int b = blockIdx.z;
    const int h0 = fuse ? 0 : (int)blockIdx.y, h1 = fuse ? heads : h0 + 1;
    const int qt = blockIdx.x * NW + wv;
    const bool live = qt * 16 < T;                        // wave-uniform
    const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
    const long ld = 3L * H;
    const float c2 = scale * LOG2E;

    f32x4 acc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int head = h0; head < h1; ++head) {
        const _Float16* base = qkv + (long)b * T * ld + head * dm;           // q at +0, k at +H, v at +2H
        if (head != h0) __syncthreads();                                      // the previous head's tiles are no longer read
        stage_f32<NKEY, D, 64 * NW>(M0, base + H, qkv_lo, ld, T, dm, tid);
        if (TWO) stage_f32<NKEY, D, 64 * NW>(M1, base + 2 * H, qkv_lo, ld, T, dm, tid);
        __syncthreads();
        if (!live) continue;

        f32x4 s[NT];
        {
            float4 qf[DG];
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int key = kt * 16 + fr;
#pragma unroll
                for (int G_ = 0; G_ < DG; ++G_) {
                    const float4 kf = *(const float4*)(M0 + key * PITCH + 16 * G_ + 4 * g);
                    MFMA4(s[kt], kf, qf[G_]);             // S^T [key][q]
                }
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (kt * 16 + g * 4 + r < T) ? s[kt][r] * c2 : -INFINITY;       // log2 domain
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = exp2f(s[kt][r] - mx); s[kt][r] = e; sum += e; }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] *= inv;                                      // P^T [key][q]; 0 for keys >= T

        if (GRAD) {
            const _Float16* dob = dctx + (long)b * T * H + head * dm;
            float4 of[DG];
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) of[G_] = grow4(dob, dctx_lo, (long)qr * H, 16 * G_ + 4 * g, dm);
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                f32x4 dp = {0.f, 0.f, 0.f, 0.f};
                const int key = kt * 16 + fr, keyc = key < T ? key : T - 1;
#pragma unroll
                for (int G_ = 0; G_ < DG; ++G_) {
                    float4 vf;
                    if (TWO) vf = *(const float4*)(M1 + key * PITCH + 16 * G_ + 4 * g);
                    else vf = grow4(base + 2 * H, qkv_lo, (long)keyc * ld, 16 * G_ + 4 * g, dm);
                    MFMA4(dp, vf, of[G_]);                // dP^T [key][q]
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = s[kt][r] * (dp[r] * dscale);
                    s[kt][r] = v < 0.f ? 0.f : v;         // (P * dP)^+; a NaN stays a NaN
                }
            }
        }

        // fold this head into the fused tile, heads in index order (a NaN wins max and min as it wins the sum)
        if (head == h0) {
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) acc[kt] = s[kt];
        } else if (fuse == 1) {
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) acc[kt] += s[kt];
        } else if (fuse == 2) {
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[kt][r] = (s[kt][r] > acc[kt][r] || s[kt][r] != s[kt][r]) ? s[kt][r] : acc[kt][r];
        } else {
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[kt][r] = (s[kt][r] < acc[kt][r] || s[kt][r] != s[kt][r]) ? s[kt][r] : acc[kt][r];
        }
    }
    if (!live || qrow >= T) return;

    const float mean = fuse == 1 ? 1.f / (float)heads : 1.f;
    float* orow = out + ((fuse ? (long)b : (long)b * heads + h0) * T + qrow) * T;
    const bool vec = (T & 3) == 0;                        // rows start 16-byte aligned
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const int key = kt * 16 + g * 4;
        if (vec) {
            if (key < T) *(float4*)(orow + key) = make_float4(acc[kt][0] * mean, acc[kt][1] * mean, acc[kt][2] * mean, acc[kt][3] * mean);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key + r < T) orow[key + r] = acc[kt][r] * mean;
        }
    }
}

template <int NT, int D, bool GRAD>
static int launch_att_maps(const void* qkv, long qkv_lo, const void* dctx, long dctx_lo, float dscale, int fuse, float* out, int B, int T,
                           int H, int heads, int dm, float scale, hipStream_t s) {
    typedef AttMaps<NT, D, GRAD> G;
    static_assert(G::LDS_BYTES <= 160 * 1024, "one staged matrix must fit");
    if (advh_ensure_lds((const void*)attention_maps_kernel<NT, D, GRAD>) != ADVH_OK) return ADVH_ELAUNCH;
    const int nt = (T + 15) / 16;
    hipLaunchKernelGGL((attention_maps_kernel<NT, D, GRAD>), dim3((nt + G::NW - 1) / G::NW, fuse ? 1 : heads, B), dim3(64 * G::NW), G::LDS_BYTES, s,
                       (const _Float16*)qkv, qkv_lo, (const _Float16*)dctx, dctx_lo, dscale, fuse, out, T, H, heads, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

// ---- rollout: Y = (alpha X + beta M X + gamma M) / (normalize ? alpha + beta rowsum(M) : 1), fp32 [B][T][T] ----------------------
// One workgroup = 16 rows x 64 columns of one clip's Y, a wavefront per 16 x 16 tile.  The contraction runs in chunks of 64:
// M[16 rows][64 k] and X[64 k][64 columns] go through LDS (zero past T), four MFMAs per chunk of 16 k.  A fifth accumulator
// multiplies M by a matrix of ones: the row sums arrive in the accumulator's own layout, summed in the same k order.
constexpr int RO_KC = 64, RO_NC = 64, RO_PITCH = 68;

__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ M, const float* __restrict__ X, float* __restrict__ Y,
                                                           float alpha, float beta, float gamma, int normalize, int T) {
    __shared__ float Ms[16 * RO_PITCH];
    __shared__ float Xs[RO_KC * RO_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.x * RO_NC, i0 = blockIdx.y * 16;
    const long mat = (long)blockIdx.z * T * T;
    const float* Mb = M + mat;
    const float* Xb = X + mat;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, rs = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < T; k0 += RO_KC) {
        if (k0) __syncthreads();
        for (int i = tid; i < 16 * RO_KC; i += 256) {
            const int r = i / RO_KC, c = i % RO_KC;
            Ms[r * RO_PITCH + c] = (i0 + r < T && k0 + c < T) ? Mb[(long)(i0 + r) * T + k0 + c] : 0.f;
        }
        for (int i = tid; i < RO_KC * RO_NC; i += 256) {
            const int r = i / RO_NC, c = i % RO_NC;
            Xs[r * RO_PITCH + c] = (k0 + r < T && j0 + c < T) ? Xb[(long)(k0 + r) * T + j0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RO_KC; k += 4) {
            const float a = Ms[fr * RO_PITCH + k + g];                       // A[i = fr][k + g]
            const float x = Xs[(k + g) * RO_PITCH + wv * 16 + fr];           // B[k + g][j = fr]
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
        const float num = alpha * Xb[o] + beta * acc[r] + gamma * Mb[o];
        Y[mat + o] = normalize ? num / (alpha + beta * rs[r]) : num;
    }
}

// rel[b][j] = (1/T) sum_i X[b][i][j]: one thread per column, rows in order
__global__ __launch_bounds__(256) void rollout_relevance_kernel(const float* __restrict__ X, float* __restrict__ rel, int T) {
    const int j = threadIdx.x, b = blockIdx.x;
    if (j >= T) return;
    const float* Xb = X + (long)b * T * T;
    float s = 0.f;
    for (int i = 0; i < T; ++i) s += Xb[(long)i * T + j];
    rel[(long)b * T + j] = s / (float)T;
}

}  // namespace advh

using namespace advh;

extern "C" int advh_attention_maps(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, float dscale, int fuse, float* out,
                                   int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !out || B <= 0 || T <= 0 || heads <= 0 || H <= 0 || H % heads) return ADVH_EINVAL;
    if (fuse < 0 || fuse > 3 || !isfinite(dscale)) return ADVH_EINVAL;
    if (qkv_lo < 0 || qkv_lo % 8) return ADVH_EINVAL;
    if (dctx && (qkv_lo ? (dctx_lo <= 0 || dctx_lo % 8) : dctx_lo != 0)) return ADVH_EINVAL;     // both split or both plain fp16
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const int D = dm <= 32 ? 32 : (dm <= 64 ? 64 : 128);
    const float scale = 1.f / sqrtf((float)dm);
    hipStream_t s = (hipStream_t)stream;
    const int nt = (T + 15) / 16;
    const long dlo = dctx ? dctx_lo : 0;
#define ATM(NT_, D_)                                                                                                        \
    return dctx ? launch_att_maps<NT_, D_, true>(qkv, qkv_lo, dctx, dlo, dscale, fuse, out, B, T, H, heads, dm, scale, s) \
                : launch_att_maps<NT_, D_, false>(qkv, qkv_lo, dctx, dlo, dscale, fuse, out, B, T, H, heads, dm, scale, s)
#define ATM_D(D_)                                                                     \
    do {                                                                              \
        if (nt <= 4) ATM(4, D_); else if (nt <= 8) ATM(8, D_); else if (nt <= 13) ATM(13, D_); else ATM(16, D_); \
    } while (0)
    if (D == 32) ATM_D(32);
    else if (D == 64) ATM_D(64);
    else ATM_D(128);
#undef ATM_D
#undef ATM
    return ADVH_EUNSUPPORTED;
}

extern "C" int advh_rollout_step(const float* M, const float* X, float* Y, float alpha, float beta, float gamma, int normalize, int B, int T,
                                 advh_stream_t stream) {
    if (!M || !X || !Y || Y == X || Y == M || B <= 0 || T <= 0) return ADVH_EINVAL;
    if (T > 256) return ADVH_EUNSUPPORTED;
    hipLaunchKernelGGL(rollout_step_kernel, dim3((T + RO_NC - 1) / RO_NC, (T + 15) / 16, B), dim3(256), 0, (hipStream_t)stream, M, X, Y, alpha,
                       beta, gamma, normalize, T);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_rollout_relevance(const float* X, float* rel, int B, int T, advh_stream_t stream) {
    if (!X || !rel || B <= 0 || T <= 0) return ADVH_EINVAL;
    if (T > 256) return ADVH_EUNSUPPORTED;
    hipLaunchKernelGGL(rollout_relevance_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, X, rel, T);
    return ADVH_LAUNCH_CHECK();
}
