// Coalition batches and the attribution sums of the Shapley attributions (Captum's ShapleyValueSampling, ShapleyValues and
// KernelShap): include/addvisor_hip.h, advh_coalition_points / advh_shapley_accumulate / advh_coalition_scatter.
//
// The coalition rows are a rule of the row-building skeleton, csrc/attribution_rows.h; the other two kernels are grid-stride
// loops with one thread per (clip, sample).  All are memory-bound and tiny next to the classifier forwards they serve.
//
// Order contract: the Shapley sum of sample (b, t) adds diff[p][rank_p(id)][b] for p = p0 .. p0 + np - 1 sequentially in
// increasing p onto the running total, and the last call divides once (__fdiv_rn), as Captum's total_attrib += eval_diff *
// mask; total_attrib / iter_count does (the steps that do not switch the sample's feature add an exact zero).  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_rows.h"
#include "common.h"

namespace advh {

enum { COAL_RANK = 0, COAL_PRESENCE = 1 };

struct CoalCtx {
    const float* x;
    const float* base;
    const int32_t* index;
    const int32_t* rank;
    const uint8_t* present;
    long n, p0, rows;
    int B, base_rows, index_rows, mode, K, P;
};

// The coalition rows (csrc/attribution_rows.h).  Rank mode: row g = ((p0 + pl) * K + j) * B + b keeps the features of rank <= j in
// permutation pl of the table; presence mode: row g keeps the features whose byte in table row g is non-zero.  Rows past the end
// of the table (rank mode: (p0 + P) * K * B, presence mode: rows) are padding.
struct CoalitionRule {
    CoalCtx c;
    __host__ __device__ long n() const { return c.n; }
    struct Row {
        long pl, j, g;
        bool pad;
        const float *xr, *br;
        const int32_t* ir;
    };
    __device__ __forceinline__ Row row(long g) const {
        const long kb = (long)c.K * c.B;
        const long first = c.mode == COAL_RANK ? c.p0 * kb : 0L, end = c.mode == COAL_RANK ? (c.p0 + c.P) * kb : c.rows;
        const long b = g % c.B, rel = g - first;
        return {rel / kb, (rel / c.B) % c.K, g, g >= end, c.x + b * c.n, c.base + (c.base_rows == 1 ? 0L : b * c.n),
                c.index + (c.index_rows == 1 ? 0L : b * c.n)};
    }
    // x when the feature `id` of a sample is in the row's coalition, the baseline when it is not, NaN for an id outside [0, K)
    __device__ __forceinline__ float pick(const Row& w, int id, float xv, float bv) const {
        if (id < 0 || id >= c.K) return NAN;
        const bool keep = c.mode == COAL_RANK ? c.rank[w.pl * c.K + id] <= w.j : c.present[w.g * c.K + id] != 0;
        return keep ? xv : bv;
    }
    __device__ __forceinline__ float4 quad(const Row& w, long t) const {
        const float4 xv = *(const float4*)(w.xr + t);
        if (w.pad) return xv;
        const float4 bv = *(const float4*)(w.br + t);
        const int4 id = *(const int4*)(w.ir + t);
        return make_float4(pick(w, id.x, xv.x, bv.x), pick(w, id.y, xv.y, bv.y), pick(w, id.z, xv.z, bv.z), pick(w, id.w, xv.w, bv.w));
    }
    __device__ __forceinline__ float one(const Row& w, long t) const { return w.pad ? w.xr[t] : pick(w, w.ir[t], w.xr[t], w.br[t]); }
};

// total[b][t] += sum_{p = p0 .. p0 + np - 1, increasing} (F(row p, j, b) - F(row p, j - 1, b)), j = rank_p(index[b][t]),
// F(row p, -1, b) = fbase[b]; fk[((p - p0) * K + j) * B + b].  fdiv > 0: total /= fdiv afterwards (one rounded division).
__global__ __launch_bounds__(256) void shapley_accumulate_kernel(CoalCtx c, const float* __restrict__ fbase, const float* __restrict__ fk,
                                                                 long p0, int np, float fdiv, float* __restrict__ total) {
    const long all = (long)c.B * c.n, kb = (long)c.K * c.B;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long)gridDim.x * 256) {
        const long b = i / c.n, t = i - b * c.n;
        const int id = c.index[(c.index_rows == 1 ? 0L : b * c.n) + t];
        float acc = total[i];
        if (id < 0 || id >= c.K) {
            acc = NAN;
        } else {
            for (int q = 0; q < np; ++q) {
                const long j = c.rank[(p0 - c.p0 + q) * c.K + id];
                if (j < 0 || j >= c.K) {                                        // not a permutation: no read past fk
                    acc = NAN;
                    break;
                }
                const float* f = fk + (long)q * kb + b;
                acc += f[j * c.B] - (j == 0 ? fbase[b] : f[(j - 1) * c.B]);
            }
        }
        total[i] = fdiv > 0.f ? __fdiv_rn(acc, fdiv) : acc;
    }
}

// attr[b][t] = coef[b][index[b][t]] (NaN for an index outside [0, K))
__global__ __launch_bounds__(256) void coalition_scatter_kernel(CoalCtx c, const float* __restrict__ coef, float* __restrict__ attr) {
    const long all = (long)c.B * c.n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long)gridDim.x * 256) {
        const long b = i / c.n, t = i - b * c.n;
        const int id = c.index[(c.index_rows == 1 ? 0L : b * c.n) + t];
        attr[i] = id >= 0 && id < c.K ? coef[b * c.K + id] : NAN;
    }
}

}  // namespace advh

using namespace advh;

// the fields every entry point reads (index map and shape); `tables`: also x, base and the mode's table
static int coalition_ctx(const advh_coalition_desc* d, bool tables, CoalCtx* c) {
    if (!d || !d->index || d->B <= 0 || d->n <= 0 || d->K <= 0) return ADVH_EINVAL;
    if (d->index_rows != 1 && d->index_rows != d->B) return ADVH_EINVAL;
    if (d->mode == COAL_RANK) {
        if (!d->rank || d->P < 0 || d->p0 < 0) return ADVH_EINVAL;
    } else if (d->mode == COAL_PRESENCE) {
        if (tables && (!d->present || d->rows < 0)) return ADVH_EINVAL;
    } else {
        return ADVH_EINVAL;
    }
    if (tables && (!d->x || !d->base || (d->base_rows != 1 && d->base_rows != d->B))) return ADVH_EINVAL;
    *c = CoalCtx{d->x, d->base, d->index, d->mode == COAL_RANK ? d->rank : nullptr, d->mode == COAL_PRESENCE ? d->present : nullptr,
                 (long)d->n, (long)d->p0, (long)d->rows, d->B, d->base_rows, d->index_rows, d->mode, d->K, d->P};
    return ADVH_OK;
}

extern "C" int advh_coalition_points(const advh_coalition_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    CoalCtx c;
    if (coalition_ctx(d, true, &c) != ADVH_OK || !out || row0 < 0 || rows < 0) return ADVH_EINVAL;
    if (c.mode == COAL_RANK && row0 < c.p0 * c.K * c.B) return ADVH_EINVAL;           // rows before the table's permutations
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.base) && aligned16(c.index) && aligned16(out);
    return build_rows(CoalitionRule{c}, vec, (long)row0, rows, out, (hipStream_t)stream);
}

extern "C" int advh_shapley_accumulate(const advh_coalition_desc* d, const float* fbase, const float* fk, int64_t p0, int np,
                                       float* total, float finalize_div, advh_stream_t stream) {
    CoalCtx c;
    if (coalition_ctx(d, false, &c) != ADVH_OK || c.mode != COAL_RANK || !fbase || !total || np < 0 || (np > 0 && !fk)) return ADVH_EINVAL;
    if (p0 < c.p0 || p0 + np > c.p0 + c.P || !(finalize_div >= 0.f) || isinf(finalize_div)) return ADVH_EINVAL;
    hipLaunchKernelGGL(shapley_accumulate_kernel, dim3(grid_for((long)c.B * c.n)), dim3(256), 0, (hipStream_t)stream, c, fbase, fk,
                       (long)p0, np, finalize_div, total);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_coalition_scatter(const advh_coalition_desc* d, const float* coef, float* attr, advh_stream_t stream) {
    CoalCtx c;
    if (coalition_ctx(d, false, &c) != ADVH_OK || !coef || !attr) return ADVH_EINVAL;
    hipLaunchKernelGGL(coalition_scatter_kernel, dim3(grid_for((long)c.B * c.n)), dim3(256), 0, (hipStream_t)stream, c, coef, attr);
    return ADVH_LAUNCH_CHECK();
}
