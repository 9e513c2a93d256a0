// Captum's attribution metrics, infidelity and sensitivity_max (include/addvisor_hip.h, advh_metric_rows / advh_metric_row_dot /
// advh_infidelity_fold / advh_infidelity_finalize / advh_row_norm / advh_sensitivity_fold): the perturbed rows of a chunk of
// samples, the per-row dot products and norms, and the per-clip folds.
//
// These kernels move ~12 B per sample per row next to a forward (or a whole attribution) per row, so they stay simple:
// grid-stride loops, one workgroup per row for the row reductions, and the quad walkers of attribution_lanes.h, which states
// the float4 / scalar rule (float4 when base pointers are aligned and n % 4 == 0; both forms visit the same elements in the same
// order and give the same bits) and the row tree.
//
// Determinism contract: the noise of element (g, j) is a pure function of (seed, g, j) with the global (clip, sample) row
// g = b * S + s0 + s' (the words of advh_philox_normal), so a row does not depend on the chunking.  Every row sum is the row tree
// in one workgroup: thread t adds the quads t, t + 256, ... in order, the four elements of a quad in order, then the tree.  The
// per-clip folds run one thread per clip, samples in increasing order.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"
#include "philox.h"

// Every product and sum below is rounded on its own: no FMA contraction, so sigma * N (and r * (2u - 1)) is rounded before
// the subtraction (addition), as the unfused torch expression of a Python perturb_func rounds it, and a product is rounded
// before it joins a row sum, as in advh_metric_row_dot.  The bit-identity of the fused and generic paths rests on this.
#pragma clang fp contract(off)

namespace advh {

enum { MR_UNIFORM = 0, MR_GAUSS = 1 };
enum { NORM_2 = 0, NORM_1 = 1, NORM_INF = 2 };

struct MetricCtx {
    const float* x;
    const float* attr;
    const float* base;
    long n;
    uint64_t seed;
    int B, S, s0, p, base_rows, mode, mul;
    float scale;
};

// One element of a perturbed row: v = x + r * (2u - 1) (uniform; 2u - 1 is exact) or v = x - sigma * z (Gaussian), and in the
// Gaussian mode its term of the dot product, pert * a, with pert = sigma * z or (multiply_by_inputs) the decorator's
// safe_div(x - v, x - b) from the rounded v.
__device__ __forceinline__ float metric_elem(const MetricCtx& c, float xv, float av, float bv, float z, float* term) {
    if (c.mode == MR_UNIFORM) return xv + c.scale * (2.f * z - 1.f);
    const float nz = c.scale * z;
    const float v = xv - nz;
    float pert = nz;
    if (c.mul) {
        const float den = c.base ? xv - bv : xv;
        pert = (xv - v) / (den != 0.f ? den : 1.f);
    }
    *term = pert * av;
    return v;
}

// Row r of a launch (chunk row rr = row0 + r, clip b = rr / p, global row g = b * S + s0 + rr % p): out[r] = the perturbed row,
// dot[rr] = sum_j pert_j * attr[b][j] (Gaussian mode).  One workgroup per row.
template <bool VEC>
__global__ __launch_bounds__(256) void metric_rows_kernel(MetricCtx c, long row0, float* __restrict__ out, float* __restrict__ dot) {
    const long rr = row0 + blockIdx.x;
    const int b = (int)(rr / c.p);
    const long g = (long)b * c.S + c.s0 + (rr - (long)b * c.p);
    const float* xr = c.x + (long)b * c.n;
    const float* ar = c.attr ? c.attr + (long)b * c.n : nullptr;
    const float* br = c.base ? c.base + (c.base_rows == 1 ? 0L : (long)b * c.n) : nullptr;
    float* orow = out + (long)blockIdx.x * c.n;
    const long nq = (c.n + 3) / 4;
    float s = 0.f;
    for (long q = threadIdx.x; q < nq; q += 256) {
        float4 z;
        if (c.mode == MR_UNIFORM) {
            const uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)g, (uint32_t)((unsigned long)g >> 32), 0u),
                                          (uint32_t)c.seed, (uint32_t)(c.seed >> 32));
            z = make_float4(philox_uniform(w.x), philox_uniform(w.y), philox_uniform(w.z), philox_uniform(w.w));
        } else {
            z = philox_normal4(c.seed, g, q);
        }
        const lanes<4> zv = {{z.x, z.y, z.z, z.w}};
        const lanes<4> xv = load_quad<VEC>(xr, q, c.n), av = load_quad_or<VEC>(ar, q, c.n), bv = load_quad_or<VEC>(br, q, c.n);
        lanes<4> o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = 0.f;
            o[k] = metric_elem(c, xv[k], av[k], bv[k], zv[k], &t);
            if (c.mode == MR_GAUSS && quad_lane<VEC>(q, k, c.n)) s = s + t;
        }
        store_quad<VEC>(orow, q, c.n, o);
    }
    if (c.mode == MR_GAUSS) {
        s = block_sum(s);
        if (threadIdx.x == 0) dot[rr] = s;
    }
}

// dot[r] = sum_j pert[r][j] * attr[r / p][j], the tree of metric_rows_kernel.  One workgroup per row.
template <bool VEC>
__global__ __launch_bounds__(256) void row_dot_kernel(const float* __restrict__ pert, const float* __restrict__ attr, int p, long n,
                                                      float* __restrict__ dot) {
    const long r = blockIdx.x;
    const float* pr = pert + r * n;
    const float* ar = attr + (r / p) * n;
    const long nq = (n + 3) / 4;
    float s = 0.f;
    for (long q = threadIdx.x; q < nq; q += 256) {
        const lanes<4> pv = load_quad<VEC>(pr, q, n), av = load_quad<VEC>(ar, q, n);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (quad_lane<VEC>(q, k, n)) s = s + pv[k] * av[k];
    }
    s = block_sum(s);
    if (threadIdx.x == 0) dot[r] = s;
}

__device__ __forceinline__ float norm_acc(float s, float d, int ord) {
    return ord == NORM_2 ? s + d * d : ord == NORM_1 ? s + fabsf(d) : nanmax(s, fabsf(d));
}

// out[r] = ||d_r||_ord with d_r = a[r] (b == NULL) or a[r / p] - b[r]; divided by div[r / p] (0 replaced by 1) when div != NULL.
// One workgroup per row; the 2-norm is the square root of the tree's sum of squares.
template <bool VEC>
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ a, const float* __restrict__ b, int p, long n, int ord,
                                                       const float* __restrict__ div, float* __restrict__ out) {
    const long r = blockIdx.x;
    const float* ar = a + (b ? r / p : r) * n;
    const float* brow = b ? b + r * n : nullptr;
    const long nq = (n + 3) / 4;
    float s = 0.f;
    for (long q = threadIdx.x; q < nq; q += 256) {
        const lanes<4> av = load_quad<VEC>(ar, q, n), bv = load_quad_or<VEC>(brow, q, n);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (quad_lane<VEC>(q, k, n)) s = norm_acc(s, brow ? av[k] - bv[k] : av[k], ord);
    }
    s = block_reduce(s, ord == NORM_INF);
    if (threadIdx.x == 0) {
        float v = ord == NORM_2 ? sqrtf(s) : s;
        if (div) {
            const float dv = div[b ? r / p : r];
            v = v / (dv == 0.f ? 1.f : dv);
        }
        out[r] = v;
    }
}

// smax[b] = max(smax[b], ratio[b * p + s]) over s = 0 .. p - 1 in order (NaN propagates); one thread per clip.
__global__ __launch_bounds__(256) void max_fold_kernel(const float* __restrict__ ratio, int B, int p, float* __restrict__ smax) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        float m = smax[b];
        for (int s = 0; s < p; ++s) m = nanmax(m, ratio[(long)b * p + s]);
        smax[b] = m;
    }
}

// Infidelity fold, one thread per clip, samples in increasing order: a = dot[b * p + s], d = f0[b] - fk[b * p + s] (an fp32
// difference of the fp32 logits, as Captum forms it); fp64 sums acc[b] += (a - d)^2, or (normalize) acc[3b .. 3b + 2] +=
// (a^2, a d, d^2), each operation rounded on its own.
__global__ __launch_bounds__(256) void infidelity_fold_kernel(const float* __restrict__ dot, const float* __restrict__ f0,
                                                              const float* __restrict__ fk, int B, int p, int normalize,
                                                              double* __restrict__ acc) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        double s0 = normalize ? acc[3L * b] : acc[b], s1 = normalize ? acc[3L * b + 1] : 0.0, s2 = normalize ? acc[3L * b + 2] : 0.0;
        for (int s = 0; s < p; ++s) {
            const long r = (long)b * p + s;
            const double a = dot[r], d = (double)(f0[b] - fk[r]);
            if (normalize) {
                s0 = __dadd_rn(s0, __dmul_rn(a, a));
                s1 = __dadd_rn(s1, __dmul_rn(a, d));
                s2 = __dadd_rn(s2, __dmul_rn(d, d));
            } else {
                const double e = __dsub_rn(a, d);
                s0 = __dadd_rn(s0, __dmul_rn(e, e));
            }
        }
        if (normalize) {
            acc[3L * b] = s0;
            acc[3L * b + 1] = s1;
            acc[3L * b + 2] = s2;
        } else {
            acc[b] = s0;
        }
    }
}

// out[b] = acc[b] / S, or (normalize) with A, AD, D = acc[3b ..]: beta = AD / (A != 0 ? A : 1),
// ((beta * beta) * A - (2 * beta) * AD) + D, then / S -- Captum's expression, each operation rounded in fp64, one rounding to fp32.
__global__ __launch_bounds__(256) void infidelity_finalize_kernel(const double* __restrict__ acc, int B, int S, int normalize,
                                                                  float* __restrict__ out) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        double v;
        if (normalize) {
            const double A = acc[3L * b], AD = acc[3L * b + 1], D = acc[3L * b + 2];
            const double beta = __ddiv_rn(AD, A != 0.0 ? A : 1.0);
            v = __dadd_rn(__dsub_rn(__dmul_rn(__dmul_rn(beta, beta), A), __dmul_rn(__dmul_rn(2.0, beta), AD)), D);
        } else {
            v = acc[b];
        }
        out[b] = (float)__ddiv_rn(v, (double)S);
    }
}

}  // namespace advh

using namespace advh;

// B * p rows must index as int (one workgroup per row)
static inline bool chunk_ok(int B, int p) { return B > 0 && p > 0 && (int64_t)B * p <= 0x7fffffff; }

extern "C" int advh_metric_rows(const advh_metric_desc* d, int64_t row0, int rows, float* out, float* dot, advh_stream_t stream) {
    if (!d || !d->x || !out || d->n <= 0 || d->S <= 0 || d->s0 < 0 || !chunk_ok(d->B, d->p) || d->p > d->S - d->s0) return ADVH_EINVAL;
    if (row0 < 0 || rows <= 0 || row0 + rows > (int64_t)d->B * d->p) return ADVH_EINVAL;
    if (!(d->scale >= 0.f) || isinf(d->scale) || (d->mul != 0 && d->mul != 1)) return ADVH_EINVAL;
    if (d->mode == MR_UNIFORM) {
        if (dot || d->mul) return ADVH_EINVAL;
    } else if (d->mode == MR_GAUSS) {
        if (!d->attr || !dot) return ADVH_EINVAL;
    } else {
        return ADVH_EINVAL;
    }
    if (d->base && d->base_rows != 1 && d->base_rows != d->B) return ADVH_EINVAL;
    const MetricCtx c{d->x, d->mode == MR_GAUSS ? d->attr : nullptr, d->mode == MR_GAUSS && d->mul ? d->base : nullptr, (long)d->n,
                      d->seed, d->B, d->S, d->s0, d->p, d->base_rows, d->mode, d->mul, d->scale};
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.attr) && aligned16(c.base) && aligned16(out);
    launch_vec(vec, metric_rows_kernel<true>, metric_rows_kernel<false>, dim3(rows), (hipStream_t)stream, c, row0, out, dot);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_metric_row_dot(const float* pert, const float* attr, int B, int p, int64_t n, float* dot, advh_stream_t stream) {
    if (!pert || !attr || !dot || !chunk_ok(B, p) || n <= 0) return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(pert) && aligned16(attr);
    launch_vec(vec, row_dot_kernel<true>, row_dot_kernel<false>, dim3(B * p), (hipStream_t)stream, pert, attr, p, n, dot);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_infidelity_fold(const float* dot, const float* f0, const float* fk, int B, int p, int normalize, double* acc,
                                    advh_stream_t stream) {
    if (!dot || !f0 || !fk || !acc || !chunk_ok(B, p) || (normalize != 0 && normalize != 1)) return ADVH_EINVAL;
    hipLaunchKernelGGL(infidelity_fold_kernel, dim3(grid_for(B)), dim3(256), 0, (hipStream_t)stream, dot, f0, fk, B, p, normalize, acc);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_infidelity_finalize(const double* acc, int B, int S, int normalize, float* out, advh_stream_t stream) {
    if (!acc || !out || B <= 0 || S <= 0 || (normalize != 0 && normalize != 1)) return ADVH_EINVAL;
    hipLaunchKernelGGL(infidelity_finalize_kernel, dim3(grid_for(B)), dim3(256), 0, (hipStream_t)stream, acc, B, S, normalize, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_row_norm(const float* v, int rows, int64_t n, int ord, float* out, advh_stream_t stream) {
    if (!v || !out || rows <= 0 || n <= 0 || ord < NORM_2 || ord > NORM_INF) return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(v);
    launch_vec(vec, row_norm_kernel<true>, row_norm_kernel<false>, dim3(rows), (hipStream_t)stream, v, nullptr, 1, n, ord, nullptr, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_sensitivity_fold(const float* e, const float* et, const float* enorm, int B, int p, int64_t n, int ord, float* ratio,
                                     float* smax, advh_stream_t stream) {
    if (!e || !et || !enorm || !ratio || !smax || !chunk_ok(B, p) || n <= 0 || ord < NORM_2 || ord > NORM_INF) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && aligned16(e) && aligned16(et);
    launch_vec(vec, row_norm_kernel<true>, row_norm_kernel<false>, dim3(B * p), s, e, et, p, n, ord, enorm, ratio);
    hipLaunchKernelGGL(max_fold_kernel, dim3(grid_for(B)), dim3(256), 0, s, (const float*)ratio, B, p, smax);
    return ADVH_LAUNCH_CHECK();
}
