// Row and waveform-end kernels of the ragged gradient chain: the ragged siblings of pool_logreg_bwd_kernel (backward.hip),
// gn0_bwd_kernel and the two wave_bwd kernels (frontend_bwd.hip), and the fp16 / plane-pair form of advh_zero_tail_rows.
//
// frames / lens: int32 [B] on the device.  Clip b has frames[b] valid rows of its T and lens[b] valid samples of its L; both are
// clamped inside the kernels (frames to [1, T] or [0, T], lens to [10, L]) so that no array content can move an access.  Clips
// stay T rows / L samples apart, the tiles (64 frames, 2048 samples) and the order of every sum are the siblings', so
// frames[b] = T / lens[b] = L reproduces the sibling bit for bit, and a shorter clip gets what the sibling gives for it run alone:
// the tiles past its end add exact zeros.  The kernels of backward.hip and frontend_bwd.hip are left exactly as they are.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"

namespace advh {
namespace ragged_bwd {

constexpr int K0 = 10, S0 = 5, TT = 64, WT = 2048;

__device__ __forceinline__ int clamp_frames(const int* __restrict__ frames, int b, int lo, int T) {
    const int f = frames[b];
    return f < lo ? lo : (f > T ? T : f);
}
__device__ __forceinline__ int clip_len(const int* __restrict__ lens, int b, int L) {
    const int l = lens[b];
    return l < K0 ? K0 : (l > L ? L : l);
}

// dh[b][t][:] = coef[:] * (dlogit[b] / Tv_b) for t < Tv_b, 0 for Tv_b <= t < T      (mean over the clip's own frames + Linear(H,1))
__global__ __launch_bounds__(256) void pool_logreg_bwd_ragged_kernel(const float* __restrict__ coef, const float* __restrict__ dlogit,
                                                                     float* __restrict__ dh, _Float16* __restrict__ dh16,
                                                                     const int* __restrict__ frames, int T, int H, long total4, long dh16_lo) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        int c = (int)(i % (H / 4)) * 4;
        long bt = i / (H / 4);
        int b = (int)(bt / T), t = (int)(bt - (long)b * T);
        const int Tv = clamp_frames(frames, b, 1, T);
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < Tv) {
            float s = dlogit[b] / Tv;
            float4 w = *(const float4*)(coef + c);
            o[0] = w.x * s; o[1] = w.y * s; o[2] = w.z * s; o[3] = w.w * s;
        }
        if (dh) *(float4*)(dh + bt * H + c) = make_float4(o[0], o[1], o[2], o[3]);
        if (dh16) store_h_rt<4>(dh16, bt * H + c, dh16_lo, o);
    }
}

// x[b, frames[b]:, :] = 0 for fp16 rows, and for the lo plane `lo` elements behind when lo != 0.  Grid row b = clip b.
// VEC: 16-byte stores (x 16-byte aligned, H % 8 == 0, lo % 8 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void zero_tail_rows_h_kernel(_Float16* __restrict__ x, long lo, const int* __restrict__ frames, int T, int H) {
    const int b = blockIdx.y, f0 = clamp_frames(frames, b, 0, T);
    _Float16* xb = x + ((long)b * T + f0) * H;
    const long n = (long)(T - f0) * H;
    const long start = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (VEC) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long i = start; i < n / 8; i += step) {
            ((float4*)xb)[i] = z;
            if (lo) ((float4*)(xb + lo))[i] = z;
        }
    } else {
        for (long i = start; i < n; i += step) {
            xb[i] = (_Float16)0.f;
            if (lo) xb[i + lo] = (_Float16)0.f;
        }
    }
}

__device__ __forceinline__ float ldn(const float* w, int i, int n, float mean, float rstd) {
    float x = i < n ? w[i] : 0.f;
    return (x - mean) * rstd;
}

// gn0_bwd_kernel with the clip's own frame count T0_b = (lens[b] - 10) / 5 + 1: the bound of the sums, the divisor of m1 / m2 and
// the bound above which dz0 is written as zero (up to P0, as the sibling writes rows [T0, P0))
template <int PASS>
__global__ __launch_bounds__(256) void gn0_bwd_ragged_kernel(const float* __restrict__ wave, long stride, int n_in, int Lmax,
                                                             const int* __restrict__ lens,
                                                             const float2* __restrict__ stats, const float* __restrict__ w0,
                                                             const float2* __restrict__ norm, const float2* __restrict__ mr,
                                                             const float* __restrict__ gamma, const _Float16* __restrict__ dy,
                                                             float2* __restrict__ part, const float2* __restrict__ sums,
                                                             _Float16* __restrict__ dz, int P0, int C0, long dy_lo, long dz_lo) {
    __shared__ float xs[TT * S0 + K0];
    const int b = blockIdx.y, t0 = blockIdx.x * TT, tid = threadIdx.x, ntile = gridDim.x;
    const int L = clip_len(lens, b, Lmax), T0 = (L - K0) / S0 + 1;
    const float* w = wave + (long)b * stride;
    const int n = n_in < L ? n_in : L;
    const float2 st = stats[b];
    for (int i = tid; i < TT * S0 + K0; i += 256) xs[i] = ldn(w, S0 * t0 + i, n, st.x, st.y);
    __syncthreads();
    const int c = 2 * tid;
    if (c >= C0) return;
    float wa[K0], wb[K0];
#pragma unroll
    for (int k = 0; k < K0; ++k) { wa[k] = w0[c * K0 + k]; wb[k] = w0[(c + 1) * K0 + k]; }
    const float2 na = norm[(long)b * C0 + c], nb = norm[(long)b * C0 + c + 1];
    const float2 ma = mr[(long)b * C0 + c], mb = mr[(long)b * C0 + c + 1];
    const float ga = gamma[c], gb = gamma[c + 1];
    float s1a = 0.f, s2a = 0.f, s1b = 0.f, s2b = 0.f;
    float m1a = 0.f, m2a = 0.f, m1b = 0.f, m2b = 0.f;
    if (PASS == 1) {
        float2 sa = sums[(long)b * C0 + c], sb = sums[(long)b * C0 + c + 1];
        m1a = sa.x / T0; m2a = sa.y / T0; m1b = sb.x / T0; m2b = sb.y / T0;
    }
    const int tend = min(TT, P0 - t0);
    for (int t = 0; t < tend; ++t) {
        const long o = ((long)b * P0 + t0 + t) * C0 + c;
        float da = 0.f, db = 0.f;
        if (t0 + t < T0) {
            float za = 0.f, zb = 0.f;
#pragma unroll
            for (int k = 0; k < K0; ++k) { float x = xs[S0 * t + k]; za = fmaf(wa[k], x, za); zb = fmaf(wb[k], x, zb); }
            float d2[2];
            load_h_rt<2>(dy, o, dy_lo, d2);
            float dna = d2[0] * gelu_grad(za * na.x + na.y) * ga;
            float dnb = d2[1] * gelu_grad(zb * nb.x + nb.y) * gb;
            float ha = (za - ma.x) * ma.y, hb = (zb - mb.x) * mb.y;
            if (PASS == 0) { s1a += dna; s2a += dna * ha; s1b += dnb; s2b += dnb * hb; }
            else { da = ma.y * (dna - m1a - ha * m2a); db = mb.y * (dnb - m1b - hb * m2b); }
        }
        if (PASS == 1) { const float dd[2] = {da, db}; store_h_rt<2>(dz, o, dz_lo, dd); }
    }
    if (PASS == 0) {
        part[((long)b * ntile + blockIdx.x) * C0 + c] = make_float2(s1a, s2a);
        part[((long)b * ntile + blockIdx.x) * C0 + c + 1] = make_float2(s1b, s2b);
    }
}

__global__ __launch_bounds__(256) void gn0_reduce_ragged_kernel(const float2* __restrict__ part, float2* __restrict__ sums, int ntile, int C0) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C0) return;
    float a = 0.f, d = 0.f;
    for (int i = 0; i < ntile; ++i) { float2 v = part[((long)b * ntile + i) * C0 + c]; a += v.x; d += v.y; }
    sums[(long)b * C0 + c] = make_float2(a, d);
}

// wave_bwd_gather_kernel over the clip's own L_b = lens[b] samples and T0_b frames: dxh[b][u] for u < L_b (the rest is never read),
// per-tile partial sums (tiles past L_b hold zeros).  Clips stay Lmax samples apart in dxh.
__global__ __launch_bounds__(256) void wave_bwd_gather_ragged_kernel(const float* __restrict__ g, const float* __restrict__ wave, long stride,
                                                                     int n_in, int Lmax, const int* __restrict__ lens,
                                                                     const float2* __restrict__ stats, float* __restrict__ dxh,
                                                                     float2* __restrict__ part, int P0) {
    __shared__ float r1[4], r2[4];
    const int b = blockIdx.y, u0 = blockIdx.x * WT, tid = threadIdx.x;
    const int L = clip_len(lens, b, Lmax), T0 = (L - K0) / S0 + 1;
    const int n = n_in < L ? n_in : L;
    const float2 st = stats[b];
    const float* w = wave + (long)b * stride;
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < WT; i += 256) {
        int u = u0 + i;
        if (u >= L) break;
        int q = u / S0, phi = u - q * S0;
        float v = 0.f;
        if (q < T0) v += g[((long)b * P0 + q) * 16 + phi];
        if (q >= 1 && q - 1 < T0) v += g[((long)b * P0 + q - 1) * 16 + phi + S0];
        dxh[(long)b * Lmax + u] = v;
        float xh = ldn(w, u, n, st.x, st.y);
        s1 += v; s2 += v * xh;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if ((tid & 63) == 0) { r1[tid >> 6] = s1; r2[tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) part[(long)b * gridDim.x + blockIdx.x] = make_float2((r1[0] + r1[1]) + (r1[2] + r1[3]), (r2[0] + r2[1]) + (r2[2] + r2[3]));
}

// dx[k] = rho (g_k - S1/L_b) - xhat_k S2 / ((L_b-1) sigma) for k < L_b, 0 for L_b <= k < n_in;   out = dx * out_scale
__global__ __launch_bounds__(256) void wave_bwd_final_ragged_kernel(const float* __restrict__ dxh, const float* __restrict__ wave, long stride,
                                                                    int n_in, int Lmax, const int* __restrict__ lens,
                                                                    const float2* __restrict__ stats, const float2* __restrict__ part,
                                                                    int npart, int normalize, float out_scale, float* __restrict__ dx,
                                                                    long dx_stride) {
    __shared__ float sh[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        float a = 0.f, d = 0.f;
        for (int i = 0; i < npart; ++i) { float2 v = part[(long)b * npart + i]; a += v.x; d += v.y; }
        sh[0] = a; sh[1] = d;
    }
    __syncthreads();
    const int L = clip_len(lens, b, Lmax);
    const float2 st = stats[b];
    const float rho = st.y, sigma = 1.f / st.y - 1e-7f;
    const float S1 = sh[0], S2 = sh[1];
    const float* w = wave + (long)b * stride;
    for (int i = tid; i < WT; i += 256) {
        int u = blockIdx.x * WT + i;
        if (u >= n_in) break;
        float v = 0.f;
        if (u < L) {
            float gk = dxh[(long)b * Lmax + u];
            if (normalize) {
                float xh = (w[u] - st.x) * rho;
                v = rho * (gk - S1 / L) - xh * S2 / ((float)(L - 1) * sigma);
            } else {
                v = gk;
            }
        }
        dx[(long)b * dx_stride + u] = v * out_scale;
    }
}

}  // namespace ragged_bwd
}  // namespace advh

using namespace advh::ragged_bwd;

static int pool_logreg_bwd_ragged_launch(const float* coef, const float* dlogit, float* dh, void* dh16, long dh16_lo, const int32_t* frames,
                                         int B, int T, int H, advh_stream_t stream) {
    if (!coef || !dlogit || !frames || (!dh && !dh16) || B <= 0 || T <= 0 || H <= 0 || H % 4) return ADVH_EINVAL;
    long total4 = (long)B * T * (H / 4);
    long blocks = (total4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pool_logreg_bwd_ragged_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, coef, dlogit, dh,
                       (_Float16*)dh16, (const int*)frames, T, H, total4, dh16_lo);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_pool_logreg_bwd_ragged(const float* coef, const float* dlogit, float* dh, void* dh16, const int32_t* frames, int B,
                                           int T, int H, advh_stream_t stream) {
    return pool_logreg_bwd_ragged_launch(coef, dlogit, dh, dh16, 0, frames, B, T, H, stream);
}

extern "C" int advh_pool_logreg_bwd_split_ragged(const float* coef, const float* dlogit, float* dh, void* dh16, int64_t dh16_lo,
                                                 const int32_t* frames, int B, int T, int H, advh_stream_t stream) {
    if (dh16 && (dh16_lo <= 0 || dh16_lo % 4)) return ADVH_EINVAL;
    return pool_logreg_bwd_ragged_launch(coef, dlogit, dh, dh16, dh16 ? dh16_lo : 0, frames, B, T, H, stream);
}

extern "C" int advh_zero_tail_rows_h(void* x, int64_t lo, const int32_t* frames, int B, int T, int H, advh_stream_t stream) {
    if (!x || !frames || lo < 0 || B <= 0 || T <= 0 || H <= 0) return ADVH_EINVAL;
    if (B > 65535) return ADVH_EUNSUPPORTED;                 // one grid row per clip
    const bool vec = aligned16(x) && H % 8 == 0 && lo % 8 == 0;
    const dim3 grid(grid_for((long)T * H / (vec ? 8 : 1), 64), B);
    launch_vec(vec, zero_tail_rows_h_kernel<true>, zero_tail_rows_h_kernel<false>, grid, (hipStream_t)stream, (_Float16*)x, (long)lo,
               (const int*)frames, T, H);
    return ADVH_LAUNCH_CHECK();
}

static int frontend_bwd_group_ragged_launch(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                            const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                            const void* dy0, long dy_lo, float* part_ws, float* sums_ws, void* dz0, long dz_lo, int T0,
                                            int P0, int C0, const int32_t* lens, advh_stream_t stream) {
    if (!wave || !w0 || !gamma || !stats_ws || !norm_ws || !mr_ws || !dy0 || !part_ws || !sums_ws || !dz0 || !lens) return ADVH_EINVAL;
    if (B <= 0 || n_in <= 0 || L < K0 || C0 <= 0 || C0 > 512 || (C0 & 1) || T0 != (L - K0) / S0 + 1 || P0 < T0) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int* lv = (const int*)lens;
    dim3 grid((P0 + TT - 1) / TT, B);
    hipLaunchKernelGGL(gn0_bwd_ragged_kernel<0>, grid, dim3(256), 0, s, wave, (long)wave_stride, n_in, L, lv, (const float2*)stats_ws, w0,
                       (const float2*)norm_ws, (const float2*)mr_ws, gamma, (const _Float16*)dy0, (float2*)part_ws, (const float2*)nullptr,
                       (_Float16*)nullptr, P0, C0, dy_lo, dz_lo);
    hipLaunchKernelGGL(gn0_reduce_ragged_kernel, dim3((C0 + 255) / 256, B), dim3(256), 0, s, (const float2*)part_ws, (float2*)sums_ws,
                       (int)grid.x, C0);
    hipLaunchKernelGGL(gn0_bwd_ragged_kernel<1>, grid, dim3(256), 0, s, wave, (long)wave_stride, n_in, L, lv, (const float2*)stats_ws, w0,
                       (const float2*)norm_ws, (const float2*)mr_ws, gamma, (const _Float16*)dy0, (float2*)nullptr, (const float2*)sums_ws,
                       (_Float16*)dz0, P0, C0, dy_lo, dz_lo);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_w2v2_frontend_bwd_group_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                                   const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                                   const void* dy0, float* part_ws, float* sums_ws, void* dz0, int T0, int P0, int C0,
                                                   const int32_t* lens, advh_stream_t stream) {
    return frontend_bwd_group_ragged_launch(wave, wave_stride, n_in, B, L, w0, gamma, stats_ws, norm_ws, mr_ws, dy0, 0, part_ws, sums_ws,
                                            dz0, 0, T0, P0, C0, lens, stream);
}

extern "C" int advh_w2v2_frontend_bwd_group_split_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                                         const float* gamma, const float* stats_ws, const float* norm_ws,
                                                         const float* mr_ws, const void* dy0, int64_t dy_lo, float* part_ws,
                                                         float* sums_ws, void* dz0, int64_t dz_lo, int T0, int P0, int C0,
                                                         const int32_t* lens, advh_stream_t stream) {
    if (dy_lo <= 0 || dz_lo <= 0 || dy_lo % 2 || dz_lo % 2) return ADVH_EINVAL;
    return frontend_bwd_group_ragged_launch(wave, wave_stride, n_in, B, L, w0, gamma, stats_ws, norm_ws, mr_ws, dy0, dy_lo, part_ws,
                                            sums_ws, dz0, dz_lo, T0, P0, C0, lens, stream);
}

extern "C" int advh_wave_bwd_ragged(const float* g, const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* stats_ws,
                                    float* dxhat_ws, float* part_ws, int normalize, float out_scale, float* dx, int64_t dx_stride,
                                    int T0, int P0, const int32_t* lens, advh_stream_t stream) {
    if (!g || !wave || !stats_ws || !dxhat_ws || !part_ws || !dx || !lens || B <= 0 || L < K0 || n_in <= 0 || dx_stride < n_in) return ADVH_EINVAL;
    if (T0 != (L - K0) / S0 + 1 || P0 < T0) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int* lv = (const int*)lens;
    const int nt = (L + WT - 1) / WT, nto = ((n_in > L ? n_in : L) + WT - 1) / WT;
    hipLaunchKernelGGL(wave_bwd_gather_ragged_kernel, dim3(nt, B), dim3(256), 0, s, g, wave, (long)wave_stride, n_in, L, lv,
                       (const float2*)stats_ws, dxhat_ws, (float2*)part_ws, P0);
    hipLaunchKernelGGL(wave_bwd_final_ragged_kernel, dim3(nto, B), dim3(256), 0, s, (const float*)dxhat_ws, wave, (long)wave_stride, n_in, L,
                       lv, (const float2*)stats_ws, (const float2*)part_ws, nt, normalize, out_scale, dx, (long)dx_stride);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_backward_ragged)
