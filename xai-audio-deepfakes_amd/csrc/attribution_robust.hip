// Captum's adversarial attacks, FGSM and PGD (include/addvisor_hip.h, advh_robust_step / advh_robust_random_start /
// advh_robust_first_flip): the iterate update between two forward + backward pairs of the gradient chain -- the signed step,
// PGD's projection onto the Linf or L2 ball around the clean clip and the bound clamp in one pass -- PGD's random start, and
// the fold of an epsilon ladder.
//
// These kernels move ~16 B per sample next to a forward + backward per row, so they stay simple, as attribution_metrics.hip: the
// quad walkers of attribution_lanes.h, which states the float4 / scalar rule (float4 when base pointers are aligned and
// n % 4 == 0; both forms visit the same elements in the same order) and the row tree.  Without a row reduction (no projection,
// Linf) a row is split over several workgroups, grid-stride over its quads; the L2 projection and the L2 random start take one
// workgroup of 256 per row.
//
// Determinism contract: an output element is a pure function of its own inputs and, for L2, of its row's norm.  The row sum of
// squares is the row tree: thread t adds the quads t, t + 256, ... in order, the four elements of a quad in order, then the tree;
// every thread reads the same four partials, so the whole row is scaled by one value.  Pass 2 recomputes the step from its inputs;
// the row is not staged.
// The random start of clip b is a pure function of (seed, b, B).  The ladder fold runs one thread per clip, k in increasing
// order.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"
#include "philox.h"

// Every product and sum below is rounded on its own: no FMA contraction, so e * sign(g) * mask is rounded before it joins x, and
// x0 + clamp(v - x0) is three roundings, as Captum's unfused torch expressions round them (tests/robust_ref.py restates them).
#pragma clang fp contract(off)

namespace advh {

enum { RN_NONE = 0, RN_LINF = 1, RN_L2 = 2 };
enum { ROBUST_MAX_P = ADVH_ROBUST_MAX_P };

struct RobustCtx {
    const float* x0;
    const float* x;
    const float* grad;
    const float* seed;
    const float* mask;
    long n;
    int p, x_per_row, grad_per_row, mask_per_clip, norm, chunks;
    float radius, lo, hi;
    float e[ROBUST_MAX_P];
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    v = v < lo ? lo : v;                                     // NaN passes through, as torch.clamp
    return v > hi ? hi : v;
}

// FGSM._perturb of one element: torch.where(|g| > zero_thresh, x + multiplier * epsilon * sign(g) * mask, x), g the loss gradient
// seed * grad (seed == 1 when has_seed is false), e = (float)(multiplier * epsilon).
__device__ __forceinline__ float fgsm_elem(float xv, float gv, float sd, bool has_seed, float e, float mv, bool has_mask) {
    const float gl = has_seed ? sd * gv : gv;
    const float sg = gl > 0.f ? 1.f : gl < 0.f ? -1.f : 0.f;
    float t = e * sg;
    if (has_mask) t = t * mv;
    return fabsf(gl) > 1e-6f ? xv + t : xv;
}

// Launch row r = row0 + blockIdx.x / chunks (clip b = r / p, ladder index k = r % p): out[r - row0] = bound(project(step)).
// L2: one workgroup per row (chunks == 1), pass 1 sums (v - x0)^2 over the tree, pass 2 recomputes v and scales.
template <bool VEC, bool L2>
__global__ __launch_bounds__(256) void robust_step_kernel(RobustCtx c, long row0, float* out) {
    const long lr = blockIdx.x / c.chunks;
    const int chunk = blockIdx.x - (int)lr * c.chunks;
    const long r = row0 + lr;
    const int b = (int)(r / c.p);
    const int k = (int)(r - (long)b * c.p);
    const float* xr = c.x + (c.x_per_row ? r : (long)b) * c.n;
    const float* gr = c.grad + (c.grad_per_row ? r : (long)b) * c.n;
    const float* x0r = c.x0 ? c.x0 + (long)b * c.n : nullptr;
    const float* mr = c.mask ? c.mask + (c.mask_per_clip ? (long)b * c.n : 0L) : nullptr;
    float* orow = out + lr * c.n;
    const bool has_seed = c.seed != nullptr, has_mask = mr != nullptr;
    const float sd = has_seed ? c.seed[b] : 1.f;
    const float e = c.e[k];
    const long nq = (c.n + 3) / 4;
    const long q0 = (long)chunk * 256 + threadIdx.x, qs = (long)c.chunks * 256;
    // the step of quad q, and its clean clip's elements (0 without a projection)
    auto step = [&](long q, lanes<4>* cv) {
        const lanes<4> xv = load_quad<VEC>(xr, q, c.n), gv = load_quad<VEC>(gr, q, c.n), mv = load_quad_or<VEC>(mr, q, c.n);
        *cv = L2 ? load_quad<VEC>(x0r, q, c.n) : load_quad_or<VEC>(x0r, q, c.n);   // a projection always has its clean clip
        lanes<4> v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fgsm_elem(xv[i], gv[i], sd, has_seed, e, mv[i], has_mask);
        return v;
    };
    float scale = 1.f;
    if (L2) {
        float s = 0.f;
        for (long q = q0; q < nq; q += qs) {
            lanes<4> cv;
            const lanes<4> v = step(q, &cv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = v[i] - cv[i];
                if (quad_lane<VEC>(q, i, c.n)) s = s + d * d;
            }
        }
        const float nrm = sqrtf(block_sum(s));               // the barrier inside: every read of pass 1 precedes pass 2's writes
        scale = nrm > c.radius ? c.radius / (nrm + 1e-7f) : 1.f;
    }
    for (long q = q0; q < nq; q += qs) {
        lanes<4> cv;
        lanes<4> v = step(q, &cv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (L2) {
                v[i] = cv[i] + (v[i] - cv[i]) * scale;
            } else if (c.norm == RN_LINF) {
                v[i] = cv[i] + clampf(v[i] - cv[i], -c.radius, c.radius);
            }
            v[i] = clampf(v[i], c.lo, c.hi);
        }
        store_quad<VEC>(orow, q, c.n, v);
    }
}

// PGD._random_point of clip b = blockIdx.x, bounded.  Linf: x0 + radius * (2u - 1), u the uniforms of Philox row b (the row of
// advh_metric_rows' uniform mode with S = 1).  L2: x0 + (r_b / ||z||) * z, z the normals of Philox row b (advh_philox_normal),
// ||z|| over the fixed tree, r_b = radius * u_b^(1/n) with u_b the first uniform of Philox row B + b.  One workgroup per clip.
template <bool VEC, bool L2>
__global__ __launch_bounds__(256) void robust_random_start_kernel(const float* x0, int B, long n, uint64_t seed, float radius, float lo,
                                                                  float hi, float* out) {
    const long b = blockIdx.x;
    const float* xr = x0 + b * n;
    float* orow = out + b * n;
    const long nq = (n + 3) / 4;
    float coef = radius;
    if (L2) {
        float s = 0.f;
        for (long q = threadIdx.x; q < nq; q += 256) {
            const float4 z = philox_normal4(seed, b, q);
            const float zk[4] = {z.x, z.y, z.z, z.w};
            for (int i = 0; i < 4; ++i) {
                if (q * 4 + i >= n) break;
                s = s + zk[i] * zk[i];
            }
        }
        const float nrm = sqrtf(block_sum(s));
        const long g = (long)B + b;
        const uint4 w = philox4x32_10(make_uint4(0u, (uint32_t)g, (uint32_t)((unsigned long)g >> 32), 0u), (uint32_t)seed,
                                      (uint32_t)(seed >> 32));
        const float rb = radius * powf(philox_uniform(w.x), 1.f / (float)n);
        coef = rb / nrm;
    }
    for (long q = threadIdx.x; q < nq; q += 256) {
        float4 z;
        if (L2) {
            z = philox_normal4(seed, b, q);
        } else {
            const uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)b, (uint32_t)((unsigned long)b >> 32), 0u), (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
            z = make_float4(2.f * philox_uniform(w.x) - 1.f, 2.f * philox_uniform(w.y) - 1.f, 2.f * philox_uniform(w.z) - 1.f,
                            2.f * philox_uniform(w.w) - 1.f);
        }
        const float zk[4] = {z.x, z.y, z.z, z.w};
        lanes<4> o = load_quad<VEC>(xr, q, n);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = clampf(o[i] + coef * zk[i], lo, hi);
        store_quad<VEC>(orow, q, n, o);
    }
}

// out[b] = eps[k], first[b] = k of the first k with (logit[b * K + k] > 0) != (clean[b] > 0); +inf and K when no k flips.  One
// thread per clip, k in increasing order.
__global__ __launch_bounds__(256) void robust_first_flip_kernel(const float* __restrict__ logit, const float* __restrict__ clean,
                                                                const float* __restrict__ eps, int B, int K, float* __restrict__ out,
                                                                int* __restrict__ first) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        const bool pos = clean[b] > 0.f;
        int k = 0;
        while (k < K && (logit[(long)b * K + k] > 0.f) == pos) ++k;
        out[b] = k < K ? eps[k] : INFINITY;
        first[b] = k;
    }
}

}  // namespace advh

using namespace advh;

static inline bool rows_ok(int rows, int B, int p) { return rows == B || (int64_t)rows == (int64_t)B * p; }

extern "C" int advh_robust_step(const advh_robust_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    if (!d || !d->x || !d->grad || !d->eps || !out || d->n <= 0 || d->B <= 0 || d->p <= 0 || d->p > ROBUST_MAX_P) return ADVH_EINVAL;
    const int64_t R = (int64_t)d->B * d->p;
    if (R > 0x7fffffff || row0 < 0 || rows <= 0 || row0 + rows > R) return ADVH_EINVAL;
    if (d->norm < RN_NONE || d->norm > RN_L2 || (d->targeted != 0 && d->targeted != 1)) return ADVH_EINVAL;
    if (!rows_ok(d->x_rows, d->B, d->p) || !rows_ok(d->grad_rows, d->B, d->p)) return ADVH_EINVAL;
    if (d->mask && d->mask_rows != 1 && d->mask_rows != d->B) return ADVH_EINVAL;
    if (!(d->lo <= d->hi)) return ADVH_EINVAL;                                 // lo > hi, or a NaN bound
    if (d->norm != RN_NONE && (!d->x0 || !(d->radius >= 0.f) || isinf(d->radius))) return ADVH_EINVAL;
    RobustCtx c{};
    for (int k = 0; k < d->p; ++k) {
        if (!(d->eps[k] >= 0.0) || isinf(d->eps[k])) return ADVH_EINVAL;
        c.e[k] = (float)((d->targeted ? -1.0 : 1.0) * d->eps[k]);              // multiplier * epsilon, a Python float, then fp32
    }
    c.x0 = d->norm != RN_NONE ? d->x0 : nullptr;
    c.x = d->x, c.grad = d->grad, c.seed = d->seed, c.mask = d->mask, c.n = (long)d->n;
    c.p = d->p, c.norm = d->norm;
    c.x_per_row = d->p > 1 && d->x_rows != d->B, c.grad_per_row = d->p > 1 && d->grad_rows != d->B;
    c.mask_per_clip = d->mask && d->mask_rows != 1;
    c.radius = d->norm != RN_NONE ? d->radius : 0.f, c.lo = d->lo, c.hi = d->hi;
    const long nq = (c.n + 3) / 4;
    long chunks = d->norm == RN_L2 ? 1 : (nq + 255) / 256;
    chunks = chunks > 64 ? 64 : chunks;
    if ((int64_t)rows * chunks > 0x7fffffff) chunks = 1;
    c.chunks = (int)chunks;
    const bool vec = c.n % 4 == 0 && aligned16(c.x0) && aligned16(c.x) && aligned16(c.grad) && aligned16(c.mask) && aligned16(out);
    const dim3 grid((unsigned)(rows * chunks));
    hipStream_t s = (hipStream_t)stream;
    if (d->norm == RN_L2)
        launch_vec(vec, robust_step_kernel<true, true>, robust_step_kernel<false, true>, grid, s, c, row0, out);
    else
        launch_vec(vec, robust_step_kernel<true, false>, robust_step_kernel<false, false>, grid, s, c, row0, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_robust_random_start(const float* x0, int B, int64_t n, uint64_t seed, int norm, float radius, float lo, float hi,
                                        float* out, advh_stream_t stream) {
    if (!x0 || !out || B <= 0 || n <= 0 || (norm != RN_LINF && norm != RN_L2)) return ADVH_EINVAL;
    if (!(radius >= 0.f) || isinf(radius) || !(lo <= hi)) return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(x0) && aligned16(out);
    const dim3 grid(B);
    hipStream_t s = (hipStream_t)stream;
    if (norm == RN_L2)
        launch_vec(vec, robust_random_start_kernel<true, true>, robust_random_start_kernel<false, true>, grid, s, x0, B, n, seed, radius, lo, hi, out);
    else
        launch_vec(vec, robust_random_start_kernel<true, false>, robust_random_start_kernel<false, false>, grid, s, x0, B, n, seed, radius, lo, hi,
                   out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_robust_first_flip(const float* logit, const float* clean_logit, const float* eps, int B, int K, float* out,
                                      int* first, advh_stream_t stream) {
    if (!logit || !clean_logit || !eps || !out || !first || B <= 0 || K <= 0 || (int64_t)B * K > 0x7fffffff) return ADVH_EINVAL;
    long blocks = ((long)B + 255) / 256;
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(robust_first_flip_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logit, clean_logit, eps, B, K,
                       out, first);
    return ADVH_LAUNCH_CHECK();
}
