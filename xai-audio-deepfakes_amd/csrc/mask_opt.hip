// Per-clip optimised mask explanations (Fong & Vedaldi 2017; Fong, Patrick & Vedaldi 2019): include/addvisor_hip.h,
// advh_mask_opt_rows / advh_mask_opt_terms / advh_mask_opt_step -- the three launches that keep the optimisation loop of
// HipSpectralAttribution.optimize_mask on the device next to the classifier's forward / backward chain.
//
//   rows  : theta [B][Fc][Tc] -> the mask rows of a chunk of whole clips, row 2j = m = U sigmoid(theta), row 2j + 1 = 1.f - m
//   terms : the regularisers A, mean p, TV of a clip (one workgroup per clip, one fixed tree), the two seeds of the chain's
//           backward from the clip's two logits, one history row, and p itself for the step kernel
//   step  : grad theta = p (1 - p) (U^T (G_in - G_out) + regulariser derivatives), one wavefront per (clip, coarse cell), and the
//           Adam / SGD update of theta in place
//
// U is torch's bilinear upsampling (align_corners = False).  Its per-axis rule, axis_weight(), is written once and used by the
// rows kernel (U) and by the step kernel (U^T and the footprint of a coarse cell), so the pair is adjoint by construction: the
// weight the step kernel gives the pair (fine bin, coarse cell) is the weight the rows kernel gave it.  p = sigmoid(theta) is one
// function too, so the three kernels see the same bits.
//
// Deterministic: no atomics, every sum in an order fixed by the geometry alone.  All three are tiny next to the chain they sit in
// (K <= a few thousand cells per clip, Fm * Tm <= 513 * T bins per row): they are written to be exact and launch-count-minimal,
// not to be tuned.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"

#pragma clang fp contract(off)                             // every product is rounded before it joins a sum: one arithmetic for both row forms

namespace advh {

enum { REWARD_LOGIT = 0, REWARD_PROB = 1, REWARD_LOG_PROB = 2, OPT_ADAM = 0, OPT_SGD = 1 };

__device__ __forceinline__ float sigmoid_f(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

// One axis of the upsampling: fine index d of N reads the coarse points i0, i1 of n with weights 1 - w1, w1.
//   src = max((d + 0.5) n / N - 0.5, 0), i0 = min(floor(src), n - 1), i1 = min(i0 + 1, n - 1), w1 = src - i0
// Evaluated in integers: 2 N src = max((2 d + 1) n - N, 0) =: num, i0 = num / (2 N), w1 = (num mod 2 N) / (2 N) -- i0 is exact and
// w1 one correctly rounded division of two integers below 2^24 (a float src of up to n carries an absolute error of n * 2^-24,
// 2e-6 at n = 33, straight into the weight).  n == N gives i0 = d and w1 = 0, an integer scale exact dyadic weights.
// src < n - 0.5, so i0 <= n - 1 without a clamp.  N <= 32768 (checked by the entry points) keeps num inside int.
struct AxisW {
    int i0, i1;
    float w1;
};
__device__ __forceinline__ AxisW axis_weight(int d, int n, int N) {
    const int num = max((2 * d + 1) * n - N, 0), den = 2 * N;
    AxisW a;
    a.i0 = num / den;
    a.i1 = min(a.i0 + 1, n - 1);
    a.w1 = __fdiv_rn((float)(num - a.i0 * den), (float)den);
    return a;
}

// the weight U gives coarse index c at fine index d on one axis (0 when d does not read c)
__device__ __forceinline__ float axis_weight_of(int d, int c, int n, int N) {
    const AxisW a = axis_weight(d, n, N);
    return (a.i0 == c ? 1.f - a.w1 : 0.f) + (a.i1 == c ? a.w1 : 0.f);
}

// The footprint [lo, hi] of coarse index c: the fine indices d with i0(d) == c or i1(d) == c.  i0 is non-decreasing in d and,
// for n <= N, takes every value of [0, n), so the set is the range from the first d with i0(d) >= c - 1 to the last d with
// i0(d) <= c.  A closed-form estimate, then verified with axis_weight itself: the loops move at most a step or two and are
// bounded by N whatever the estimate.
__device__ __forceinline__ void axis_footprint(int c, int n, int N, int& lo, int& hi) {
    const float s = __fdiv_rn((float)N, (float)n);
    int l = (int)floorf(((float)c - 0.5f) * s - 0.5f);
    int h = (int)ceilf(((float)c + 1.5f) * s - 0.5f);
    l = max(0, min(l, N - 1));
    h = max(0, min(h, N - 1));
    for (int g = 0; g < N && l > 0 && axis_weight(l - 1, n, N).i0 >= c - 1; ++g) --l;
    for (int g = 0; g < N && l < N - 1 && axis_weight(l, n, N).i0 < c - 1; ++g) ++l;
    for (int g = 0; g < N && h < N - 1 && axis_weight(h + 1, n, N).i0 <= c; ++g) ++h;
    for (int g = 0; g < N && h > 0 && axis_weight(h, n, N).i0 > c; ++g) --h;
    lo = l;
    hi = h;
}

// m[f][t] of one clip: the sigmoid at the four coarse corners, the lerp along t, then along f.
__device__ __forceinline__ float mask_at(const float* __restrict__ th, int f, int t, const advh_mask_opt_desc& c) {
    const AxisW af = axis_weight(f, c.Fc, c.Fm), at = axis_weight(t, c.Tc, c.Tm);
    const float* r0 = th + (long)af.i0 * c.Tc;
    const float* r1 = th + (long)af.i1 * c.Tc;
    const float a = sigmoid_f(r0[at.i0]) * (1.f - at.w1) + sigmoid_f(r0[at.i1]) * at.w1;
    const float b = sigmoid_f(r1[at.i0]) * (1.f - at.w1) + sigmoid_f(r1[at.i1]) * at.w1;
    return a * (1.f - af.w1) + b * af.w1;
}

// rows[2j][q] = m_{b0 + j}[q], rows[2j + 1][q] = 1.f - rows[2j][q]; item i of the grid-stride loop is W consecutive bins of one clip
template <bool VEC>
__global__ __launch_bounds__(256) void mask_opt_rows_kernel(advh_mask_opt_desc c, const float* __restrict__ theta, int b0, int nb,
                                                            float* __restrict__ rows) {
    constexpr int W = VEC ? 4 : 1;
    const long n = (long)c.Fm * c.Tm, per = n / W, total = (long)nb * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long j = i / per, q = (i - j * per) * W;
        const float* th = theta + (b0 + j) * (long)c.Fc * c.Tc;
        const int f = (int)(q / c.Tm), t = (int)(q - (long)f * c.Tm);      // VEC: Tm % 4 == 0, the four bins share f
        lanes<W> m, o;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            m[k] = mask_at(th, f, t + k, c);
            o[k] = 1.f - m[k];
        }
        store_lanes<W>(rows + (2 * j) * n + q, m);
        store_lanes<W>(rows + (2 * j + 1) * n + q, o);
    }
}

// One workgroup per clip j of the chunk (clip b = b0 + j).  Thread i adds the cells i, i + 256, ... in that order, then one
// 256-leaf tree per term in LDS (tf_pool_kernel's); thread 0 forms the rewards, the seeds and the history row.
__global__ __launch_bounds__(256) void mask_opt_terms_kernel(advh_mask_opt_desc c, const float* __restrict__ theta,
                                                             const int32_t* __restrict__ rank, const float* __restrict__ sign,
                                                             const float* __restrict__ logits, int b0, float* __restrict__ p_out,
                                                             float* __restrict__ seeds, float* __restrict__ hist) {
    __shared__ float part[3][256];
    const int tid = threadIdx.x, j = blockIdx.x, b = b0 + j, K = c.Fc * c.Tc;
    const float* th = theta + (long)b * K;
    const int32_t* rk = rank + (long)b * K;
    float area = 0.f, l1 = 0.f, tv = 0.f;
    for (int k = tid; k < K; k += 256) {
        const int i = k / c.Tc, jt = k - i * c.Tc;
        const float p = sigmoid_f(th[k]);
        p_out[(long)b * K + k] = p;
        const float d = p - (rk[k] >= K - c.K1 ? 1.f : 0.f);
        area += d * d;
        l1 += p;
        if (i + 1 < c.Fc) {
            const float df = sigmoid_f(th[k + c.Tc]) - p;
            tv += df * df;
        }
        if (jt + 1 < c.Tc) {
            const float dt = sigmoid_f(th[k + 1]) - p;
            tv += dt * dt;
        }
    }
    part[0][tid] = area;
    part[1][tid] = l1;
    part[2][tid] = tv;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            part[0][tid] += part[0][tid + h];
            part[1][tid] += part[1][tid + h];
            part[2][tid] += part[2][tid + h];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float invK = __fdiv_rn(1.f, (float)K);
    const float A = part[0][0] * invK, P = part[1][0] * invK, TV = part[2][0] * invK;
    const float s = sign[b], z_in = s * logits[2 * j], z_out = s * logits[2 * j + 1];
    float phi[2], dphi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float z = q ? z_out : z_in, sg = sigmoid_f(z);
        if (c.reward == REWARD_LOGIT) {
            phi[q] = z;
            dphi[q] = 1.f;
        } else if (c.reward == REWARD_PROB) {
            phi[q] = sg;
            dphi[q] = sg * (1.f - sg);
        } else {                                           // log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)); its slope sigmoid(-z)
            phi[q] = fminf(z, 0.f) - log1pf(expf(-fabsf(z)));
            dphi[q] = sigmoid_f(-z);
        }
    }
    seeds[2 * j] = -c.lam_in * s * dphi[0];
    seeds[2 * j + 1] = c.lam_out * s * dphi[1];
    float* h = hist + (long)b * 6;
    h[0] = z_in;
    h[1] = z_out;
    h[2] = A;
    h[3] = P;
    h[4] = TV;
    h[5] = -c.lam_in * phi[0] + c.lam_out * phi[1] + c.lam_area * A + c.lam_l1 * P + c.lam_tv * TV;
}

// One wavefront per (clip j of the chunk, coarse cell k); four wavefronts per workgroup.  The lanes walk the cell's footprint box
// row-major, e = lane, lane + 64, ..., each adding (w_f w_t) (G_in - G_out) in that order; a fixed xor butterfly sums the 64
// partials (every lane ends with the same bits); lane 0 adds the regulariser derivatives from p (the terms kernel's, so no wave
// reads a theta another wave is updating), multiplies by p (1 - p), stores the gradient and updates theta and the state.
__global__ __launch_bounds__(256) void mask_opt_step_kernel(advh_mask_opt_desc c, float* __restrict__ theta, const float* __restrict__ p_in,
                                                            const int32_t* __restrict__ rank, const float* __restrict__ G, int b0, int nb,
                                                            float step_size, float bc2_sqrt, float* __restrict__ m1, float* __restrict__ m2,
                                                            float* __restrict__ grad_theta) {
    const int lane = threadIdx.x & 63, K = c.Fc * c.Tc;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (long)nb * K) return;                      // wave-uniform: whole wavefronts leave
    const int j = (int)(wave / K), k = (int)(wave - (long)j * K), b = b0 + j;
    const int ci = k / c.Tc, cj = k - ci * c.Tc;
    int f_lo, f_hi, t_lo, t_hi;
    axis_footprint(ci, c.Fc, c.Fm, f_lo, f_hi);
    axis_footprint(cj, c.Tc, c.Tm, t_lo, t_hi);
    const long n = (long)c.Fm * c.Tm;
    const float* gi = G + (2L * j) * n;
    const float* go = gi + n;
    const int tw = t_hi - t_lo + 1, box = (f_hi - f_lo + 1) * tw;
    float acc = 0.f;
    for (int e = lane; e < box; e += 64) {
        const int f = f_lo + e / tw, t = t_lo + e % tw;
        const float w = axis_weight_of(f, ci, c.Fc, c.Fm) * axis_weight_of(t, cj, c.Tc, c.Tm);
        const long q = (long)f * c.Tm + t;
        acc += w * (gi[q] - go[q]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane != 0) return;
    const float* pb = p_in + (long)b * K;
    const float p = pb[k], invK = __fdiv_rn(1.f, (float)K);
    const float r = rank[(long)b * K + k] >= K - c.K1 ? 1.f : 0.f;
    float dtv = 0.f;
    if (ci > 0) dtv += p - pb[k - c.Tc];
    if (ci + 1 < c.Fc) dtv -= pb[k + c.Tc] - p;
    if (cj > 0) dtv += p - pb[k - 1];
    if (cj + 1 < c.Tc) dtv -= pb[k + 1] - p;
    float g = acc + c.lam_area * (2.f * invK * (p - r)) + c.lam_l1 * invK + c.lam_tv * (2.f * invK * dtv);
    g = p * (1.f - p) * g;
    const long idx = (long)b * K + k;
    if (grad_theta) grad_theta[idx] = g;
    if (c.optimizer == OPT_ADAM) {                         // torch.optim.Adam: 1 - beta is formed in double, then rounded (0.999f is not 0.999)
        const float b1 = (float)c.beta1, b2 = (float)c.beta2, omb1 = (float)(1.0 - c.beta1), omb2 = (float)(1.0 - c.beta2);
        const float m = b1 * m1[idx] + omb1 * g;
        const float v = b2 * m2[idx] + omb2 * (g * g);
        m1[idx] = m;
        m2[idx] = v;
        const float denom = __fdiv_rn(sqrtf(v), bc2_sqrt) + (float)c.eps;
        theta[idx] = theta[idx] - step_size * __fdiv_rn(m, denom);
    } else {
        const float v = (float)c.momentum * m1[idx] + g;
        m1[idx] = v;
        theta[idx] = theta[idx] - step_size * v;
    }
}

}  // namespace advh

using namespace advh;

// the descriptor alone, and the clip range of a chunk
static bool mask_opt_ok(const advh_mask_opt_desc* d, int b0, int nb) {
    if (!d || d->B <= 0 || d->B > 65535 || d->Fm <= 0 || d->Tm <= 0 || d->Fc <= 0 || d->Tc <= 0) return false;
    if (d->Fc > d->Fm || d->Tc > d->Tm || d->Fm > 32768 || d->Tm > 32768) return false;
    if ((long)d->B * d->Fc * d->Tc > 0x7fffffffL) return false;   // int cell and wave numbers
    if (d->K1 < 0 || d->K1 > d->Fc * d->Tc) return false;
    if (d->reward < REWARD_LOGIT || d->reward > REWARD_LOG_PROB) return false;
    if (d->optimizer != OPT_ADAM && d->optimizer != OPT_SGD) return false;
    if (!isfinite(d->lr)) return false;
    return b0 >= 0 && nb > 0 && b0 <= d->B - nb;
}

extern "C" int advh_mask_opt_rows(const advh_mask_opt_desc* d, const float* theta, int b0, int nb, float* rows, advh_stream_t stream) {
    if (!mask_opt_ok(d, b0, nb) || !theta || !rows) return ADVH_EINVAL;
    const bool vec = d->Tm % 4 == 0 && aligned16(rows);
    const long n = (long)d->Fm * d->Tm;
    launch_vec(vec, mask_opt_rows_kernel<true>, mask_opt_rows_kernel<false>, dim3(grid_for((long)nb * (vec ? n / 4 : n))),
               (hipStream_t)stream, *d, theta, b0, nb, rows);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_mask_opt_terms(const advh_mask_opt_desc* d, const float* theta, const int32_t* rank, const float* sign,
                                   const float* logits, int b0, int nb, float* p, float* seeds, float* hist, advh_stream_t stream) {
    if (!mask_opt_ok(d, b0, nb) || !theta || !rank || !sign || !logits || !p || !seeds || !hist) return ADVH_EINVAL;
    hipLaunchKernelGGL(mask_opt_terms_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, *d, theta, rank, sign, logits, b0, p, seeds,
                       hist);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_mask_opt_step(const advh_mask_opt_desc* d, float* theta, const float* p, const int32_t* rank, const float* G, int b0,
                                  int nb, double bias1, double bias2, float* m1, float* m2, float* grad_theta, advh_stream_t stream) {
    if (!mask_opt_ok(d, b0, nb) || !theta || !p || !rank || !G || !m1) return ADVH_EINVAL;
    if (d->optimizer == OPT_ADAM && (!m2 || !(bias1 > 0.0) || !(bias2 > 0.0) || !isfinite(bias1) || !isfinite(bias2))) return ADVH_EINVAL;
    const long waves = (long)nb * d->Fc * d->Tc;
    hipLaunchKernelGGL(mask_opt_step_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *d, theta, p, rank, G,
                       b0, nb, (float)(d->optimizer == OPT_ADAM ? d->lr / bias1 : d->lr), (float)sqrt(bias2 > 0.0 ? bias2 : 1.0), m1, m2,
                       grad_theta);
    return ADVH_LAUNCH_CHECK();
}
