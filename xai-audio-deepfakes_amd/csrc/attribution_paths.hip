// Path points, accumulation and Gaussian noise of the baseline-aware attributions (IntegratedGradients with a baseline,
// GradientShap): include/addvisor_hip.h, advh_attr_path_points / advh_attr_path_accumulate / advh_philox_normal; and the
// moments of NoiseTunnel (advh_nt_fold / advh_nt_finalize), whose noisy rows are advh_attr_path_points' x~.
//
// Every kernel here is elementwise or a row reduction over fp32 rows (~40 MB per 160-row chunk at 4 s, next to hundreds of
// milliseconds of GEMMs per chunk), so they stay simple: grid-stride loops over the element walkers of attribution_lanes.h, which
// states the float4 / scalar rule (float4 when base pointers are aligned and n % 4 == 0) and the row tree.
//
// Determinism contract: the noise of element (g, j) is a pure function of (seed, g, j) -- Philox4x32-10 keyed by the seed,
// counter (j / 4, g lo, g hi, 0), Box-Muller on the four words -- so a row's values depend on neither the grid nor the
// chunking; each clip's rows of a chunk are added in global-row order by one thread per element, and every row sum is the
// row tree (attribution_lanes.h) in one workgroup.  NoiseTunnel's fp64 moments add each element's samples in increasing sample order, one
// thread per element.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"
#include "philox.h"

namespace advh {

__device__ __forceinline__ float pick(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

struct PathCtx {
    const float* x;
    const float* base;
    const int32_t* bidx;
    long n;
    uint64_t seed;
    int B, S, base_rows, clip_major;
    float sigma;
};

__device__ __forceinline__ int clip_of(const PathCtx& c, long g) { return c.clip_major ? (int)(g / c.S) : (int)(g % c.B); }

// baseline row of global row g; NULL for a gathered index outside [0, base_rows) (the caller then writes NaN: the attribution's
// finiteness check reports it instead of a read out of bounds)
__device__ __forceinline__ const float* base_of(const PathCtx& c, long g, int clip) {
    if (c.bidx) {
        const int i = c.bidx[g];
        return (i >= 0 && i < c.base_rows) ? c.base + (long)i * c.n : nullptr;
    }
    return c.base + (c.base_rows == 1 ? 0L : (long)clip * c.n);
}

// x~ - b of the W elements starting at column j of row g (W == 4: j % 4 == 0, row pointers 16-byte aligned); *bv = b there
template <int W>
__device__ __forceinline__ lanes<W> diff(const PathCtx& c, long g, int clip, const float* b, long j, lanes<W>* bv) {
    lanes<W> xv = load_lanes<W>(c.x + (long)clip * c.n + j), d;
    *bv = load_lanes<W>(b + j);
    if (c.sigma != 0.f) {
        const float4 z = philox_normal4(c.seed, g, j >> 2);
#pragma unroll
        for (int k = 0; k < W; ++k) xv[k] += c.sigma * pick(z, W == 4 ? k : (int)(j & 3));
    }
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = xv[k] - (*bv)[k];
    return d;
}

// out[r][:] = b + alpha[g] * (x~ - b),  g = row0 + r
template <bool VEC>
__global__ __launch_bounds__(256) void path_points_kernel(PathCtx c, const float* __restrict__ alpha, long row0, int rows,
                                                          float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const long per = c.n / W, total = (long)rows * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per, g = row0 + r;
        const int clip = clip_of(c, g);
        const float* b = base_of(c, g, clip);
        const float a = alpha[g];
        lanes<W> o = fill_lanes<W>(NAN), bv;
        if (b) {
            const lanes<W> d = diff<W>(c, g, clip, b, q * W, &bv);
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = bv[k] + a * d[k];
        }
        store_lanes<W>(out + r * c.n + q * W, o);
    }
}

enum { ACC_IG = 0, ACC_SHAP = 1, ACC_SHAP_GRAD = 2, FIN_IG = 3, FIN_MEAN = 4 };

// Chunk accumulation: element (clip, j) of `total` adds the chunk's rows of that clip in global-row order,
//   ACC_IG:        total += w[g] * grad[r]            (step-major rows, g % B = clip; product rounded before the add, as
//                                                      advh_scale_rows does, so a zero baseline reproduces the zero-baseline IG)
//   ACC_SHAP:      total += (x~ - b) * grad[r]        (clip-major rows, g / S = clip; x~ recomputed from the counter; the product
//                                                      rounded before the add as well, in both forms)
//   ACC_SHAP_GRAD: total += grad[r]
// clips [c0, c0 + nclip) are the ones the chunk touches.
template <bool VEC>
__global__ __launch_bounds__(256) void path_accumulate_kernel(PathCtx c, const float* __restrict__ grad, const float* __restrict__ w,
                                                              int mode, long row0, int rows, int c0, int nclip, float* __restrict__ tot) {
    constexpr int W = VEC ? 4 : 1;
    const long per = c.n / W, total = (long)nclip * per, gend = row0 + rows;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long k = i / per, q = i - k * per;
        const int clip = c0 + (int)k;
        long g, step, last;
        if (c.clip_major) {
            g = row0 > (long)clip * c.S ? row0 : (long)clip * c.S;
            last = gend < (long)(clip + 1) * c.S ? gend : (long)(clip + 1) * c.S;
            step = 1;
        } else {
            g = row0 + ((clip - row0 % c.B) % c.B + c.B) % c.B;
            last = gend;
            step = c.B;
        }
        float* tp = tot + (long)clip * c.n + q * W;
        lanes<W> acc = load_lanes<W>(tp);
        for (; g < last; g += step) {
#pragma clang fp contract(off)                             // every term is rounded before it joins the sum (diff() keeps its own rule)
            const lanes<W> gv = load_lanes<W>(grad + (g - row0) * c.n + q * W);
            if (mode == ACC_IG) {
                const float wg = w[g];
#pragma unroll
                for (int l = 0; l < W; ++l) acc[l] += wg * gv[l];
            } else if (mode == ACC_SHAP_GRAD) {
#pragma unroll
                for (int l = 0; l < W; ++l) acc[l] += gv[l];
            } else {
                const float* b = base_of(c, g, clip);
                lanes<W> bv, d = fill_lanes<W>(NAN);
                if (b) d = diff<W>(c, g, clip, b, q * W, &bv);
#pragma unroll
                for (int l = 0; l < W; ++l) acc[l] += d[l] * gv[l];
            }
        }
        store_lanes<W>(tp, acc);
    }
}

// Finalize, row r = clip r:  FIN_IG: out = (x - b) * total;  FIN_MEAN: out = total / S
template <bool VEC>
__global__ __launch_bounds__(256) void path_finalize_kernel(PathCtx c, const float* __restrict__ tot, int mode, float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const long per = c.n / W, total = (long)c.B * per;
    const float S = (float)c.S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per;
        const float* b = c.base + (c.base_rows == 1 ? 0L : r * c.n);
        const lanes<W> t = load_lanes<W>(tot + r * c.n + q * W);
        lanes<W> o;
        if (mode == FIN_IG) {
            const lanes<W> xv = load_lanes<W>(c.x + r * c.n + q * W), bv = load_lanes<W>(b + q * W);
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = (xv[k] - bv[k]) * t[k];
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = t[k] / S;
        }
        store_lanes<W>(out + r * c.n + q * W, o);
    }
}

// One workgroup per row, the row tree: sum[g] = sum_j (x~ - b)_j * v[r][j] (use_diff) or sum_j v[r][j]; g = row0 + r.  A thread
// adds one term per element in the scalar form and one four-term sum per quad in the float4 form.
template <bool VEC>
__global__ __launch_bounds__(256) void path_row_sum_kernel(PathCtx c, const float* __restrict__ v, long row0, int use_diff,
                                                           float* __restrict__ sum) {
    constexpr int W = VEC ? 4 : 1;
    const long r = blockIdx.x, g = row0 + r;
    const int clip = use_diff ? clip_of(c, g) : 0;
    const float* b = use_diff ? base_of(c, g, clip) : nullptr;
    const float* vr = v + r * c.n;
    float s = 0.f;
    if (use_diff && !b) {
        s = NAN;
    } else {
        for (long q = threadIdx.x; q < c.n / W; q += 256) {
            lanes<W> t = load_lanes<W>(vr + q * W);
            if (use_diff) {
                lanes<W> bv;
                const lanes<W> d = diff<W>(c, g, clip, b, q * W, &bv);
#pragma unroll
                for (int k = 0; k < W; ++k) t[k] = d[k] * t[k];
            }
            if constexpr (W == 4)
                s += t[0] + t[1] + t[2] + t[3];
            else
                s += t[0];
        }
    }
    s = block_sum(s);
    if (threadIdx.x == 0) sum[g] = s;
}

// out[r][j] = N(seed, row0 + r, j), or (raw) the Philox word j % 4 of counter (j / 4, row0 + r) as its bit pattern
template <bool VEC>
__global__ __launch_bounds__(256) void philox_normal_kernel(uint64_t seed, long row0, int rows, long n, int raw, float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const long per = n / W, total = (long)rows * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per, g = row0 + r, quad = VEC ? q : q >> 2;
        float4 v;
        if (raw) {
            const uint4 u = philox4x32_10(make_uint4((uint32_t)quad, (uint32_t)g, (uint32_t)((unsigned long)g >> 32), 0u), (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
            v = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
        } else {
            v = philox_normal4(seed, g, quad);
        }
        lanes<W> o;
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = pick(v, VEC ? k : (int)(q & 3));
        store_lanes<W>(out + r * n + q * W, o);
    }
}

enum { NT_SMOOTHGRAD = 0, NT_SMOOTHGRAD_SQ = 1, NT_VARGRAD = 2 };

// NoiseTunnel fold: element (b, j) adds the partition's p attributions a = attr[b * p + s][j], s = 0 .. p - 1 in increasing
// order, to the running fp64 sums of a and a * a (exact: a product of two fp32 fits a double's mantissa)
__global__ __launch_bounds__(256) void nt_fold_kernel(const float* __restrict__ attr, int B, int p, long n, double* __restrict__ sum,
                                                      double* __restrict__ sumsq) {
    const long total = (long)B * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / n, j = i - b * n;
        const float* a = attr + b * p * n + j;
        double s = sum[i], q = sumsq[i];
        for (int k = 0; k < p; ++k) {
            const double v = a[(long)k * n];
            s = __dadd_rn(s, v);
            q = __dadd_rn(q, __dmul_rn(v, v));
        }
        sum[i] = s;
        sumsq[i] = q;
    }
}

// NoiseTunnel finalize: m = sum / S, m2 = sumsq / S; out = m (smoothgrad), m2 (smoothgrad_sq), m2 - m * m (vargrad), each
// operation rounded on its own in fp64, then one rounding to fp32
__global__ __launch_bounds__(256) void nt_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ sumsq, long total,
                                                          int S, int nt_type, float* __restrict__ out) {
    const double dS = (double)S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const double m = __ddiv_rn(sum[i], dS), m2 = __ddiv_rn(sumsq[i], dS);
        out[i] = (float)(nt_type == NT_SMOOTHGRAD ? m : nt_type == NT_SMOOTHGRAD_SQ ? m2 : __dsub_rn(m2, __dmul_rn(m, m)));
    }
}

}  // namespace advh

using namespace advh;

static int path_ctx(const advh_path_desc* d, PathCtx* c) {
    if (!d || !d->x || !d->base || d->B <= 0 || d->S <= 0 || d->n <= 0 || d->base_rows <= 0 || (d->clip_major != 0 && d->clip_major != 1))
        return ADVH_EINVAL;
    if (!d->bidx && d->base_rows != 1 && d->base_rows != d->B) return ADVH_EINVAL;
    if (!(d->sigma >= 0.f) || isinf(d->sigma)) return ADVH_EINVAL;
    *c = PathCtx{d->x, d->base, d->bidx, (long)d->n, d->seed, d->B, d->S, d->base_rows, d->clip_major, d->sigma};
    return ADVH_OK;
}

static bool rows_ok(const advh_path_desc* d, int64_t row0, int rows) {
    return row0 >= 0 && rows > 0 && row0 + rows <= (int64_t)d->B * d->S;
}

extern "C" int advh_attr_path_points(const advh_path_desc* d, const float* alpha, int64_t row0, int rows, float* out, advh_stream_t stream) {
    PathCtx c;
    if (path_ctx(d, &c) != ADVH_OK || !alpha || !out || !rows_ok(d, row0, rows)) return ADVH_EINVAL;
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.base) && aligned16(out);
    const unsigned grid = grid_for((long)rows * (vec ? c.n / 4 : c.n));
    launch_vec(vec, path_points_kernel<true>, path_points_kernel<false>, dim3(grid), (hipStream_t)stream, c, alpha, row0, rows, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_attr_path_accumulate(const advh_path_desc* d, const float* grad, const float* w, int mode, int64_t row0, int rows,
                                         float* total, float* row_sum, advh_stream_t stream) {
    PathCtx c;
    if (path_ctx(d, &c) != ADVH_OK || !grad || !total || mode < ACC_IG || mode > FIN_MEAN) return ADVH_EINVAL;
    if (mode == ACC_IG && (!w || d->clip_major || row_sum)) return ADVH_EINVAL;
    if ((mode == ACC_SHAP || mode == ACC_SHAP_GRAD) && !d->clip_major) return ADVH_EINVAL;
    if (mode >= FIN_IG && (row0 != 0 || rows != d->B || (mode == FIN_IG && d->bidx) || (mode == FIN_MEAN && row_sum))) return ADVH_EINVAL;
    if (mode < FIN_IG && !rows_ok(d, row0, rows)) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.base) && aligned16(grad) && aligned16(total);
    const long per = vec ? c.n / 4 : c.n;
    if (mode >= FIN_IG) {
        launch_vec(vec, path_finalize_kernel<true>, path_finalize_kernel<false>, dim3(grid_for(c.B * per)), s, c, grad, mode, total);
        if (row_sum)                                       // per-clip sums of the attribution (IG's convergence delta)
            launch_vec(vec, path_row_sum_kernel<true>, path_row_sum_kernel<false>, dim3(c.B), s, c, total, 0L, 0, row_sum);
        return ADVH_LAUNCH_CHECK();
    }
    int c0, nclip;
    if (c.clip_major) {
        c0 = (int)(row0 / c.S);
        nclip = (int)((row0 + rows - 1) / c.S) - c0 + 1;
    } else {                                               // step-major: a clip without a row in the chunk adds nothing
        c0 = 0;
        nclip = c.B;
    }
    launch_vec(vec, path_accumulate_kernel<true>, path_accumulate_kernel<false>, dim3(grid_for(nclip * per)), s, c, grad, w, mode, row0, rows,
               c0, nclip, total);
    if (row_sum)                                           // per-row (x~ - b) . grad (GradientShap's convergence delta)
        launch_vec(vec, path_row_sum_kernel<true>, path_row_sum_kernel<false>, dim3(rows), s, c, grad, row0, 1, row_sum);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_philox_normal(uint64_t seed, int64_t row0, int rows, int64_t n, int raw, float* out, advh_stream_t stream) {
    if (!out || row0 < 0 || rows <= 0 || n <= 0 || (raw != 0 && raw != 1)) return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(out);
    const unsigned grid = grid_for((long)rows * (vec ? n / 4 : n));
    launch_vec(vec, philox_normal_kernel<true>, philox_normal_kernel<false>, dim3(grid), (hipStream_t)stream, seed, row0, rows, n, raw, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_nt_fold(const float* attr, int B, int p, int64_t n, double* sum, double* sumsq, advh_stream_t stream) {
    if (!attr || !sum || !sumsq || B <= 0 || p <= 0 || n <= 0) return ADVH_EINVAL;
    hipLaunchKernelGGL(nt_fold_kernel, dim3(grid_for((long)B * n)), dim3(256), 0, (hipStream_t)stream, attr, B, p, (long)n, sum, sumsq);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_nt_finalize(const double* sum, const double* sumsq, int B, int64_t n, int S, int nt_type, float* out,
                                advh_stream_t stream) {
    if (!sum || !sumsq || !out || B <= 0 || n <= 0 || S <= 0 || nt_type < NT_SMOOTHGRAD || nt_type > NT_VARGRAD) return ADVH_EINVAL;
    hipLaunchKernelGGL(nt_finalize_kernel, dim3(grid_for((long)B * n)), dim3(256), 0, (hipStream_t)stream, sum, sumsq, (long)B * n, S,
                       nt_type, out);
    return ADVH_LAUNCH_CHECK();
}
