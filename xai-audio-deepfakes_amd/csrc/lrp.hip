// Conservative propagation through the transformer encoder (Ali et al., ICML 2022, "XAI for Transformers: Better Explanations
// through Conservative Propagation"; the GELU identity rule of AttnLRP, Achtibat et al. 2024): gradient x input through a locally
// linearised copy of the network.  Restated from the publications -- neither Captum nor the reference has the method.  The three
// rules are three backward kernels that treat one factor of the forward as a constant:
//
//   advh_attention_bwd_value       AH-rule: ctx = sg(P) V, so dV = P^T dO and dQ = dK = 0
//   advh_layernorm_bwd_frozen(_split)  LN-rule: y = gamma (x - mean(x)) / sg(sigma) + beta, so dx = u - mean(u), u = gamma dy rstd
//   advh_gelu_identity_bwd         GELU(x) = x sg(Phi(x)), so d <- d Phi(g1)
//
// The value-only attention backward is the statistics half of pass A and the dV half of pass B of attention_bwd_f32.hip, with the
// same operand layouts: one workgroup per (clip, head), four wavefronts, both products on v_mfma_f32_16x16x4_f32 for both operand
// formats (planes joined to fp32 when staged).
//   pass 1 (wavefront = 16-query tile, scores transposed [key][q]): a query's row lives in one lane column, so row max and
//          1 / row sum are two xor-shuffles each; they go to LDS for all T queries;
//   pass 2 (wavefront = 16-key tile, scores [q][key]): the tile's dV^T [d][key] accumulators stay in registers while the wavefront
//          walks the query tiles in index order: P is recomputed from the saved statistics and goes from the score registers
//          straight into the B operand of dV^T += dO^T P.
// No atomics: every dV element has one owner and one summation order, so results are bit-identical from run to run and do not
// depend on B.  LDS holds K (pass 1) / Q (pass 2) as fp32 [NKEY][D + 4] and, when two matrices fit, dO next to it; otherwise dO
// takes the place of K after pass 1 and pass 2 fetches its Q rows from global memory.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"
#include "attention_f32_tiles.h"

namespace advh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int NT, int D>
struct AttValue {
    static constexpr int NKEY = NT * 16, PITCH = D + 4, DG = D / 16;
    static constexpr int MAT = NKEY * PITCH;                                         // floats of one staged matrix
    static constexpr bool TWO = (2 * MAT + 2 * NKEY) * 4 <= 160 * 1024;
    static constexpr int LDS_BYTES = ((TWO ? 2 : 1) * MAT + 2 * NKEY) * 4;
};

template <int NT, int D>
__global__ __launch_bounds__(256) void attention_bwd_value_kernel(const _Float16* __restrict__ qkv, long qkv_lo, const _Float16* __restrict__ dctx,
                                                                  long dctx_lo, _Float16* __restrict__ dqkv, long dqkv_lo, int T, int H, int dm,
                                                                  float scale) {
    typedef AttValue<NT, D> G;
    constexpr int NKEY = G::NKEY, PITCH = G::PITCH, DG = G::DG, NW = 4;
    constexpr bool TWO = G::TWO;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* M0 = smf;                                      // K (pass 1); pass 2: Q (TWO) or dO
    float* MO = TWO ? smf + G::MAT : smf;                 // dO of pass 2
    float* rmax = smf + (TWO ? 2 : 1) * G::MAT;
    float* rinv = rmax + NKEY;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;           // q at +0, k at +H, v at +2H
    const _Float16* dob = dctx + (long)b * T * H + head * dm;
    _Float16* dbase = dqkv + (long)b * T * ld + head * dm;
    const float c2 = scale * LOG2E;

    // dQ = dK = 0: this head's columns of the Q and K thirds, every row of the clip, both planes
    {
        const int chm = dm / 8;
        const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < T * chm; i += 64 * NW) {
            const long o = (long)(i / chm) * ld + (i % chm) * 8;
            *(f16x8*)(dbase + o) = z8;
            *(f16x8*)(dbase + o + H) = z8;
            if (dqkv_lo) {
                *(f16x8*)(dbase + o + dqkv_lo) = z8;
                *(f16x8*)(dbase + o + H + dqkv_lo) = z8;
            }
        }
    }

    stage_f32<NKEY, D, 64 * NW>(M0, base + H, qkv_lo, ld, T, dm, tid);
    if (TWO) stage_f32<NKEY, D, 64 * NW>(MO, dob, dctx_lo, (long)H, T, dm, tid);
    __syncthreads();

    // ------------------------------------------------------------------ pass 1: row max and 1 / row sum of every query
    for (int qt = wv; qt * 16 < T; qt += NW) {
        const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
        float4 qf[DG];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
        f32x4 s[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int key = kt * 16 + fr;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(M0 + key * PITCH + 16 * G_ + 4 * g);
                MFMA4(s[kt], kf, qf[G_]);                 // S^T [key][q]
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
            for (int r = 0; r < 4; ++r) sum += exp2f(s[kt][r] - mx);
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (g == 0) { rmax[qrow] = mx; rinv[qrow] = 1.f / sum; }          // qrow < NKEY: qt < NT
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass 2: dV^T [d][key] = dO^T P per key tile
    if (TWO) stage_f32<NKEY, D, 64 * NW>(M0, base, qkv_lo, ld, T, dm, tid);          // Q over K
    else stage_f32<NKEY, D, 64 * NW>(MO, dob, dctx_lo, (long)H, T, dm, tid);         // dO over K
    __syncthreads();
    for (int kt = wv; kt * 16 < T; kt += NW) {
        const int krow = kt * 16 + fr, kr_ = krow < T ? krow : T - 1;
        float4 kf[DG];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) kf[G_] = grow4(base + H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
        f32x4 dvt[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qt = 0; qt * 16 < T; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                float4 qa;
                if (TWO) qa = *(const float4*)(M0 + qrow * PITCH + 16 * G_ + 4 * g);
                else qa = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
                MFMA4(s, qa, kf[G_]);                     // S [q][key]
            }
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qt * 16 + g * 4 + r;        // this lane's query rows; its key column = krow
                p[r] = (q < T && krow < T) ? exp2f(s[r] * c2 - rmax[q]) * rinv[q] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* orw = MO + (qt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt) dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(orw[16 * dt], p[r], dvt[dt], 0, 0, 0);
            }
        }
        if (krow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                const float vv[4] = {dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]};
                store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);      // checked split conversion
            }
        }
    }
}

template <int NT, int D>
static int launch_att_value(const void* qkv, long qkv_lo, const void* dctx, long dctx_lo, void* dqkv, long dqkv_lo, int B, int T, int H,
                            int heads, int dm, float scale, hipStream_t s) {
    typedef AttValue<NT, D> G;
    static_assert(G::LDS_BYTES <= 160 * 1024, "one staged matrix must fit");
    if (advh_ensure_lds((const void*)attention_bwd_value_kernel<NT, D>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((attention_bwd_value_kernel<NT, D>), dim3(heads, B), dim3(256), G::LDS_BYTES, s, (const _Float16*)qkv, qkv_lo,
                       (const _Float16*)dctx, dctx_lo, (_Float16*)dqkv, dqkv_lo, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------- frozen-sigma LayerNorm backward
// y = gamma (x - mean(x)) sg(rstd) + beta:  dx = rstd (g - mean(g)),  g = gamma dy  (then dx += add).  One wavefront per row; the
// row statistics are those of layernorm_bwd_kernel (backward.hip), recomputed from x in the same order: rstd is the same bits.
__device__ __forceinline__ float lrp_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool F32>
__device__ __forceinline__ void lrp_load4(const void* p, long off, float (&v)[4], long lo) {
    if (F32) {
        float4 t = *(const float4*)((const float*)p + off);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        load_h_rt<4>((const _Float16*)p, off, lo, v);
    }
}

template <bool X32, bool DY32, int MAXV>
__global__ __launch_bounds__(256) void layernorm_bwd_frozen_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                                   const float* __restrict__ gamma, const float* __restrict__ add,
                                                                   float* __restrict__ out_f, _Float16* __restrict__ out_h, int M, int C,
                                                                   float eps, long x_lo, long dy_lo, long out_lo) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float xv[MAXV][4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = (i * 64 + lane) * 4;
        if (c < C) {
            lrp_load4<X32>(x, row * C + c, xv[i], x_lo);
            s += (xv[i][0] + xv[i][1]) + (xv[i][2] + xv[i][3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) xv[i][r] = 0.f;
        }
    }
    const float mean = lrp_wsum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = (i * 64 + lane) * 4;
        if (c < C) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { float d = xv[i][r] - mean; q += d * d; }
        }
    }
    const float rstd = rsqrtf(lrp_wsum(q) / C + eps);
    float sg = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {                       // xv now holds g = gamma dy
        int c = (i * 64 + lane) * 4;
        if (c < C) {
            float d[4];
            lrp_load4<DY32>(dy, row * C + c, d, dy_lo);
            const float4 gm = *(const float4*)(gamma + c);
            xv[i][0] = d[0] * gm.x; xv[i][1] = d[1] * gm.y; xv[i][2] = d[2] * gm.z; xv[i][3] = d[3] * gm.w;
            sg += (xv[i][0] + xv[i][1]) + (xv[i][2] + xv[i][3]);
        }
    }
    const float mg = lrp_wsum(sg) / C;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = (i * 64 + lane) * 4;
        if (c < C) {
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = rstd * (xv[i][r] - mg);
            if (add) {
                float4 a = *(const float4*)(add + row * C + c);
                o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
            }
            if (out_f) *(float4*)(out_f + row * C + c) = make_float4(o[0], o[1], o[2], o[3]);
            if (out_h) store_h_rt<4>(out_h, row * C + c, out_lo, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------- GELU identity rule
// out = d * Phi(g1), Phi(x) = (1 + erf(x / sqrt 2)) / 2 from fast_erf; fp16 (lo == 0) or plane pairs joined, multiplied in fp32
// and re-split through the checked conversion.  One thread per 8 elements, the n % 8 tail (and every element when a pointer or a
// plane distance is not 16-byte aligned) one by one.  out may be d.
__device__ __forceinline__ float lrp_phi(float x) { return 0.5f * (1.f + fast_erf(x * 0.70710678118654752440f)); }

template <bool VEC>
__global__ __launch_bounds__(256) void gelu_identity_bwd_kernel(const _Float16* d, long d_lo, const _Float16* __restrict__ g1, long g1_lo,
                                                                _Float16* out, long out_lo, long n) {
    const long nv = VEC ? n / 8 : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        float dv[8], gv[8];
        load_h_rt<8>(d, i * 8, d_lo, dv);
        load_h_rt<8>(g1, i * 8, g1_lo, gv);
#pragma unroll
        for (int r = 0; r < 8; ++r) dv[r] *= lrp_phi(gv[r]);
        store_h_rt<8>(out, i * 8, out_lo, dv);
    }
    for (long i = nv * 8 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float dv = d_lo ? join_f32(d[i], d[i + d_lo]) : (float)d[i];
        const float gv = g1_lo ? join_f32(g1[i], g1[i + g1_lo]) : (float)g1[i];
        const float o = dv * lrp_phi(gv);
        store_h1(out, i, out_lo, o);
    }
}

}  // namespace advh

using namespace advh;

extern "C" int advh_attention_bwd_value(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                        int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || B <= 0 || T <= 0 || heads <= 0 || H <= 0 || H % heads) return ADVH_EINVAL;
    if (qkv_lo < 0 || qkv_lo % 8) return ADVH_EINVAL;
    if (qkv_lo ? (dctx_lo <= 0 || dctx_lo % 8 || dqkv_lo <= 0 || dqkv_lo % 8) : (dctx_lo != 0 || dqkv_lo != 0)) return ADVH_EINVAL;   // all split or all fp16
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const int D = dm <= 32 ? 32 : (dm <= 64 ? 64 : 128);
    const float scale = 1.f / sqrtf((float)dm);
    hipStream_t s = (hipStream_t)stream;
    const int nt = (T + 15) / 16;
#define ATV(NT_, D_) return launch_att_value<NT_, D_>(qkv, qkv_lo, dctx, dctx_lo, dqkv, dqkv_lo, B, T, H, heads, dm, scale, s)
#define ATV_D(D_)                                                                     \
    do {                                                                              \
        if (nt <= 4) ATV(4, D_); else if (nt <= 8) ATV(8, D_); else if (nt <= 13) ATV(13, D_); else ATV(16, D_); \
    } while (0)
    if (D == 32) ATV_D(32);
    else if (D == 64) ATV_D(64);
    else ATV_D(128);
#undef ATV_D
#undef ATV
    return ADVH_EUNSUPPORTED;
}

static int layernorm_bwd_frozen_launch(const void* x, int x_is_f32, const void* dy, int dy_is_f32, const float* gamma, const float* add,
                                       float* out_f, void* out_h, int M, int C, float eps, long x_lo, long dy_lo, long out_lo,
                                       advh_stream_t stream) {
    if (!x || !dy || !gamma || (!out_f && !out_h) || M <= 0 || C <= 0 || C % 4) return ADVH_EINVAL;
    if (C > 64 * 4 * 8) return ADVH_EUNSUPPORTED;
    dim3 grid((M + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
#define LNF(X32, D32, MV)                                                                                             \
    hipLaunchKernelGGL((layernorm_bwd_frozen_kernel<X32, D32, MV>), grid, block, 0, s, x, dy, gamma, add, out_f, (_Float16*)out_h, M, C, \
                       eps, x_lo, dy_lo, out_lo)
#define LNF_MV(MV)                                                                                                    \
    do {                                                                                                              \
        if (x_is_f32 && dy_is_f32) LNF(true, true, MV); else if (x_is_f32) LNF(true, false, MV);                      \
        else if (dy_is_f32) LNF(false, true, MV); else LNF(false, false, MV);                                         \
    } while (0)
    if (C <= 64 * 4 * 2) LNF_MV(2); else if (C <= 64 * 4 * 4) LNF_MV(4); else LNF_MV(8);
#undef LNF_MV
#undef LNF
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_layernorm_bwd_frozen(const void* x, int x_is_f32, const void* dy, int dy_is_f32, const float* gamma, const float* add,
                                         float* out_f, void* out_h, int M, int C, float eps, advh_stream_t stream) {
    return layernorm_bwd_frozen_launch(x, x_is_f32, dy, dy_is_f32, gamma, add, out_f, out_h, M, C, eps, 0, 0, 0, stream);
}

extern "C" int advh_layernorm_bwd_frozen_split(const void* x, int x_is_f32, int64_t x_lo, const void* dy, int dy_is_f32, int64_t dy_lo,
                                               const float* gamma, const float* add, float* out_f, void* out_h, int64_t out_lo, int M,
                                               int C, float eps, advh_stream_t stream) {
    if ((!x_is_f32 && x_lo <= 0) || (!dy_is_f32 && dy_lo <= 0) || (out_h && out_lo <= 0)) return ADVH_EINVAL;
    if (x_lo % 4 || dy_lo % 4 || out_lo % 4) return ADVH_EINVAL;
    return layernorm_bwd_frozen_launch(x, x_is_f32, dy, dy_is_f32, gamma, add, out_f, out_h, M, C, eps, x_is_f32 ? 0 : x_lo,
                                       dy_is_f32 ? 0 : dy_lo, out_h ? out_lo : 0, stream);
}

extern "C" int advh_gelu_identity_bwd(const void* d, int64_t d_lo, const void* g1, int64_t g1_lo, void* out, int64_t out_lo, int64_t n,
                                      advh_stream_t stream) {
    if (!d || !g1 || !out || n <= 0) return ADVH_EINVAL;
    if (d_lo < 0 || (d_lo ? (g1_lo < n || out_lo < n || d_lo < n) : (g1_lo != 0 || out_lo != 0))) return ADVH_EINVAL;   // all planes or all fp16
    const bool vec = !(((uintptr_t)d | (uintptr_t)g1 | (uintptr_t)out) & 15) && !((d_lo | g1_lo | out_lo) & 7);
    long blocks = ((vec ? n / 8 + n % 8 : n) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipStream_t s = (hipStream_t)stream;
    launch_vec(vec, gelu_identity_bwd_kernel<true>, gelu_identity_bwd_kernel<false>, dim3((unsigned)blocks), s, d, d_lo, g1, g1_lo, out, out_lo, n);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_lrp)
