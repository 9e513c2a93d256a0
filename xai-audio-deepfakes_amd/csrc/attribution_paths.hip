// Path points, accumulation and Gaussian noise of the baseline-aware attributions (IntegratedGradients with a baseline,
// GradientShap): include/addvisor_hip.h, advh_attr_path_points / advh_attr_path_accumulate / advh_philox_normal; and the
// moments of NoiseTunnel (advh_nt_fold / advh_nt_finalize), whose noisy rows are advh_attr_path_points' x~.
//
// Every kernel here is elementwise or a row reduction over fp32 rows (~40 MB per 160-row chunk at 4 s, next to hundreds of
// milliseconds of GEMMs per chunk), so they stay simple: grid-stride loops, float4 access when every row pointer is 16-byte
// aligned (base pointers aligned and n % 4 == 0), a scalar path otherwise.
//
// Determinism contract: the noise of element (g, j) is a pure function of (seed, g, j) -- Philox4x32-10 keyed by the seed,
// counter (j / 4, g lo, g hi, 0), Box-Muller on the four words -- so a row's values depend on neither the grid nor the
// chunking; each clip's rows of a chunk are added in global-row order by one thread per element, and every row sum is a
// fixed-shape tree in one workgroup.  NoiseTunnel's fp64 moments add each element's samples in increasing sample order, one
// thread per element.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
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

// x~ - b of the quad starting at column j (j % 4 == 0, row pointers 16-byte aligned)
__device__ __forceinline__ float4 diff4(const PathCtx& c, long g, int clip, const float* b, long j, float4* bv) {
    float4 xv = *(const float4*)(c.x + (long)clip * c.n + j);
    *bv = *(const float4*)(b + j);
    if (c.sigma != 0.f) {
        const float4 z = philox_normal4(c.seed, g, j >> 2);
        xv.x += c.sigma * z.x, xv.y += c.sigma * z.y, xv.z += c.sigma * z.z, xv.w += c.sigma * z.w;
    }
    return make_float4(xv.x - bv->x, xv.y - bv->y, xv.z - bv->z, xv.w - bv->w);
}

__device__ __forceinline__ float diff1(const PathCtx& c, long g, int clip, const float* b, long j, float* bv) {
    float xv = c.x[(long)clip * c.n + j];
    *bv = b[j];
    if (c.sigma != 0.f) xv += c.sigma * pick(philox_normal4(c.seed, g, j >> 2), (int)(j & 3));
    return xv - *bv;
}

// out[r][:] = b + alpha[g] * (x~ - b),  g = row0 + r
template <bool VEC>
__global__ __launch_bounds__(256) void path_points_kernel(PathCtx c, const float* __restrict__ alpha, long row0, int rows,
                                                          float* __restrict__ out) {
    const long per = VEC ? c.n / 4 : c.n, total = (long)rows * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per, g = row0 + r;
        const int clip = clip_of(c, g);
        const float* b = base_of(c, g, clip);
        const float a = alpha[g];
        if (VEC) {
            float4 o = make_float4(NAN, NAN, NAN, NAN), bv;
            if (b) {
                const float4 d = diff4(c, g, clip, b, q * 4, &bv);
                o = make_float4(bv.x + a * d.x, bv.y + a * d.y, bv.z + a * d.z, bv.w + a * d.w);
            }
            *(float4*)(out + r * c.n + q * 4) = o;
        } else {
            float o = NAN, bv;
            if (b) {
                const float d = diff1(c, g, clip, b, q, &bv);
                o = bv + a * d;
            }
            out[r * c.n + q] = o;
        }
    }
}

enum { ACC_IG = 0, ACC_SHAP = 1, ACC_SHAP_GRAD = 2, FIN_IG = 3, FIN_MEAN = 4 };

// Chunk accumulation: element (clip, j) of `total` adds the chunk's rows of that clip in global-row order,
//   ACC_IG:        total += w[g] * grad[r]            (step-major rows, g % B = clip; product rounded before the add, as
//                                                      advh_scale_rows does, so a zero baseline reproduces the zero-baseline IG)
//   ACC_SHAP:      total += (x~ - b) * grad[r]        (clip-major rows, g / S = clip; x~ recomputed from the counter)
//   ACC_SHAP_GRAD: total += grad[r]
// clips [c0, c0 + nclip) are the ones the chunk touches.
template <bool VEC>
__global__ __launch_bounds__(256) void path_accumulate_kernel(PathCtx c, const float* __restrict__ grad, const float* __restrict__ w,
                                                              int mode, long row0, int rows, int c0, int nclip, float* __restrict__ tot) {
    const long per = VEC ? c.n / 4 : c.n, total = (long)nclip * per, gend = row0 + rows;
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
        if (VEC) {
            float4* tp = (float4*)(tot + (long)clip * c.n + q * 4);
            float4 acc = *tp;
            for (; g < last; g += step) {
                const float4 gv = *(const float4*)(grad + (g - row0) * c.n + q * 4);
                if (mode == ACC_IG) {
                    const float wg = w[g];
                    acc.x += __fmul_rn(wg, gv.x), acc.y += __fmul_rn(wg, gv.y), acc.z += __fmul_rn(wg, gv.z), acc.w += __fmul_rn(wg, gv.w);
                } else if (mode == ACC_SHAP_GRAD) {
                    acc.x += gv.x, acc.y += gv.y, acc.z += gv.z, acc.w += gv.w;
                } else {
                    const float* b = base_of(c, g, clip);
                    float4 bv, d = make_float4(NAN, NAN, NAN, NAN);
                    if (b) d = diff4(c, g, clip, b, q * 4, &bv);
                    acc.x += d.x * gv.x, acc.y += d.y * gv.y, acc.z += d.z * gv.z, acc.w += d.w * gv.w;
                }
            }
            *tp = acc;
        } else {
            float* tp = tot + (long)clip * c.n + q;
            float acc = *tp;
            for (; g < last; g += step) {
                const float gv = grad[(g - row0) * c.n + q];
                if (mode == ACC_IG) {
                    acc += __fmul_rn(w[g], gv);
                } else if (mode == ACC_SHAP_GRAD) {
                    acc += gv;
                } else {
                    const float* b = base_of(c, g, clip);
                    float bv;
                    acc += (b ? diff1(c, g, clip, b, q, &bv) : NAN) * gv;
                }
            }
            *tp = acc;
        }
    }
}

// Finalize, row r = clip r:  FIN_IG: out = (x - b) * total;  FIN_MEAN: out = total / S
template <bool VEC>
__global__ __launch_bounds__(256) void path_finalize_kernel(PathCtx c, const float* __restrict__ tot, int mode, float* __restrict__ out) {
    const long per = VEC ? c.n / 4 : c.n, total = (long)c.B * per;
    const float S = (float)c.S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per;
        const float* b = c.base + (c.base_rows == 1 ? 0L : r * c.n);
        if (VEC) {
            const float4 t = *(const float4*)(tot + r * c.n + q * 4);
            float4 o;
            if (mode == FIN_IG) {
                const float4 xv = *(const float4*)(c.x + r * c.n + q * 4), bv = *(const float4*)(b + q * 4);
                o = make_float4((xv.x - bv.x) * t.x, (xv.y - bv.y) * t.y, (xv.z - bv.z) * t.z, (xv.w - bv.w) * t.w);
            } else {
                o = make_float4(t.x / S, t.y / S, t.z / S, t.w / S);
            }
            *(float4*)(out + r * c.n + q * 4) = o;
        } else {
            const float t = tot[r * c.n + q];
            out[r * c.n + q] = mode == FIN_IG ? (c.x[r * c.n + q] - b[q]) * t : t / S;
        }
    }
}

// One workgroup per row, fixed-shape tree: sum[g] = sum_j (x~ - b)_j * v[r][j] (use_diff) or sum_j v[r][j]; g = row0 + r.
template <bool VEC>
__global__ __launch_bounds__(256) void path_row_sum_kernel(PathCtx c, const float* __restrict__ v, long row0, int use_diff,
                                                           float* __restrict__ sum) {
    __shared__ float red[4];
    const long r = blockIdx.x, g = row0 + r;
    const int clip = use_diff ? clip_of(c, g) : 0;
    const float* b = use_diff ? base_of(c, g, clip) : nullptr;
    const float* vr = v + r * c.n;
    float s = 0.f;
    if (use_diff && !b) {
        s = NAN;
    } else if (VEC) {
        for (long q = threadIdx.x; q < c.n / 4; q += 256) {
            const float4 t = *(const float4*)(vr + q * 4);
            if (use_diff) {
                float4 bv;
                const float4 d = diff4(c, g, clip, b, q * 4, &bv);
                s += d.x * t.x + d.y * t.y + d.z * t.z + d.w * t.w;
            } else {
                s += t.x + t.y + t.z + t.w;
            }
        }
    } else {
        for (long j = threadIdx.x; j < c.n; j += 256) {
            float bv;
            s += use_diff ? diff1(c, g, clip, b, j, &bv) * vr[j] : vr[j];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sum[g] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[r][j] = N(seed, row0 + r, j), or (raw) the Philox word j % 4 of counter (j / 4, row0 + r) as its bit pattern
template <bool VEC>
__global__ __launch_bounds__(256) void philox_normal_kernel(uint64_t seed, long row0, int rows, long n, int raw, float* __restrict__ out) {
    const long per = VEC ? n / 4 : n, total = (long)rows * per;
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
        if (VEC)
            *(float4*)(out + r * n + q * 4) = v;
        else
            out[r * n + q] = pick(v, (int)(q & 3));
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
    if (vec)
        hipLaunchKernelGGL(path_points_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, c, alpha, (long)row0, rows, out);
    else
        hipLaunchKernelGGL(path_points_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, c, alpha, (long)row0, rows, out);
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
        if (vec)
            hipLaunchKernelGGL(path_finalize_kernel<true>, dim3(grid_for(c.B * per)), dim3(256), 0, s, c, grad, mode, total);
        else
            hipLaunchKernelGGL(path_finalize_kernel<false>, dim3(grid_for(c.B * per)), dim3(256), 0, s, c, grad, mode, total);
        if (row_sum) {                                     // per-clip sums of the attribution (IG's convergence delta)
            if (vec)
                hipLaunchKernelGGL(path_row_sum_kernel<true>, dim3(c.B), dim3(256), 0, s, c, (const float*)total, 0L, 0, row_sum);
            else
                hipLaunchKernelGGL(path_row_sum_kernel<false>, dim3(c.B), dim3(256), 0, s, c, (const float*)total, 0L, 0, row_sum);
        }
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
    if (vec)
        hipLaunchKernelGGL(path_accumulate_kernel<true>, dim3(grid_for(nclip * per)), dim3(256), 0, s, c, grad, w, mode, (long)row0, rows,
                           c0, nclip, total);
    else
        hipLaunchKernelGGL(path_accumulate_kernel<false>, dim3(grid_for(nclip * per)), dim3(256), 0, s, c, grad, w, mode, (long)row0, rows,
                           c0, nclip, total);
    if (row_sum) {                                         // per-row (x~ - b) . grad (GradientShap's convergence delta)
        if (vec)
            hipLaunchKernelGGL(path_row_sum_kernel<true>, dim3(rows), dim3(256), 0, s, c, grad, (long)row0, 1, row_sum);
        else
            hipLaunchKernelGGL(path_row_sum_kernel<false>, dim3(rows), dim3(256), 0, s, c, grad, (long)row0, 1, row_sum);
    }
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_philox_normal(uint64_t seed, int64_t row0, int rows, int64_t n, int raw, float* out, advh_stream_t stream) {
    if (!out || row0 < 0 || rows <= 0 || n <= 0 || (raw != 0 && raw != 1)) return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(out);
    const unsigned grid = grid_for((long)rows * (vec ? n / 4 : n));
    if (vec)
        hipLaunchKernelGGL(philox_normal_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, seed, (long)row0, rows, (long)n, raw, out);
    else
        hipLaunchKernelGGL(philox_normal_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, seed, (long)row0, rows, (long)n, raw, out);
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
