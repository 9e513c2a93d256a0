// Ablated batches and the attribution sums of the perturbation attributions (Captum's Occlusion and FeatureAblation):
// include/addvisor_hip.h, advh_ablation_points / advh_ablation_accumulate.
//
// The ablated rows are a rule of the row-building skeleton, csrc/attribution_rows.h; the accumulation is one grid-stride loop
// with one thread per (clip, sample).  Both are memory-bound and tiny next to the K classifier forwards they serve.
//
// Order contract: the Occlusion sum of sample (b, t) adds diff[k][b] for k = k_lo .. k_hi sequentially in increasing k from
// 0.f and divides by the count, as Captum's total_attrib += diff * mask; weights += mask; total_attrib / weights does (adding
// an exact zero for the windows that do not cover t changes nothing).  No prefix sums, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_rows.h"
#include "common.h"

namespace advh {

enum { ABL_OCCLUSION = 0, ABL_FEATURE = 1 };

struct AblCtx {
    const float* x;
    const float* base;
    const int32_t* mask;
    long n;
    int B, base_rows, mask_rows, mode, win, stride, K;
};

// The ablated rows (csrc/attribution_rows.h): row g = k * B + b is x[b] with the baseline where sample t is in window / feature k;
// rows g >= K * B are padding, copies of x.
struct AblationRule {
    AblCtx c;
    __host__ __device__ long n() const { return c.n; }
    struct Row {
        long k;   // < 0: a padding row
        const float *xr, *br;
        const int32_t* mr;
    };
    __device__ __forceinline__ Row row(long g) const {
        const long b = g % c.B, k = g < (long)c.K * c.B ? g / c.B : -1L;
        return {k, c.x + b * c.n, c.base + (c.base_rows == 1 ? 0L : b * c.n),
                c.mode == ABL_FEATURE ? c.mask + (c.mask_rows == 1 ? 0L : b * c.n) : nullptr};
    }
    // Which of the samples t .. t + N - 1 the baseline replaces (bit j: sample t + j).  The N = 4 form reads the feature indices
    // as one int4 (t % 4 == 0, mask row 16-byte aligned).
    template <int N>
    __device__ __forceinline__ unsigned ablated(const Row& w, long t) const {
        if (w.k < 0) return 0u;
        unsigned bits = 0u;
        if (c.mode == ABL_OCCLUSION) {
            const long lo = w.k * c.stride;
#pragma unroll
            for (int j = 0; j < N; ++j) bits |= (t + j >= lo && t + j < lo + c.win) ? 1u << j : 0u;
        } else if (N == 4) {
            const int4 m = *(const int4*)(w.mr + t);
            bits = (m.x == w.k ? 1u : 0u) | (m.y == w.k ? 2u : 0u) | (m.z == w.k ? 4u : 0u) | (m.w == w.k ? 8u : 0u);
        } else {
            bits = w.mr[t] == w.k ? 1u : 0u;
        }
        return bits;
    }
    __device__ __forceinline__ float4 quad(const Row& w, long t) const {
        const unsigned m = ablated<4>(w, t);
        const float4 xv = *(const float4*)(w.xr + t), bv = *(const float4*)(w.br + t);
        return make_float4(m & 1u ? bv.x : xv.x, m & 2u ? bv.y : xv.y, m & 4u ? bv.z : xv.z, m & 8u ? bv.w : xv.w);
    }
    __device__ __forceinline__ float one(const Row& w, long t) const { return ablated<1>(w, t) ? w.br[t] : w.xr[t]; }
};

// attr[b][t] from f0 = F(x) [B] and fk = F(ablated) [K * B], one thread per (b, t):
//   Occlusion:       (sum_{k = k_lo..k_hi} (f0[b] - fk[k * B + b]), increasing k) / (k_hi - k_lo + 1)
//   FeatureAblation: f0[b] - fk[mask[t] * B + b]  (NaN for a mask entry outside [0, K))
__global__ __launch_bounds__(256) void ablation_accumulate_kernel(AblCtx c, const float* __restrict__ f0, const float* __restrict__ fk,
                                                                  float* __restrict__ attr) {
    const long total = (long)c.B * c.n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / c.n, t = i - b * c.n;
        const float fb = f0[b];
        float a;
        if (c.mode == ABL_OCCLUSION) {
            const long k_lo = t < c.win ? 0L : (t - c.win + c.stride) / c.stride;     // ceil((t - win + 1) / stride)
            const long k_hi = min((long)c.K - 1, t / c.stride);
            float acc = 0.f;
            for (long k = k_lo; k <= k_hi; ++k) acc += fb - fk[k * c.B + b];
            a = __fdiv_rn(acc, (float)(k_hi - k_lo + 1));
        } else {
            const int m = c.mask[(c.mask_rows == 1 ? 0L : b * c.n) + t];
            a = (m >= 0 && m < c.K) ? fb - fk[(long)m * c.B + b] : NAN;
        }
        attr[i] = a;
    }
}

}  // namespace advh

using namespace advh;

static int ablation_ctx(const advh_ablation_desc* d, AblCtx* c) {
    if (!d || !d->x || !d->base || d->B <= 0 || d->n <= 0 || d->K <= 0) return ADVH_EINVAL;
    if (d->base_rows != 1 && d->base_rows != d->B) return ADVH_EINVAL;
    if (d->mode == ABL_OCCLUSION) {
        if (d->win < 1 || d->stride < 1 || d->win > d->n || (d->stride > d->win && d->win < d->n)) return ADVH_EINVAL;
        if (d->K != (d->n - d->win + d->stride - 1) / d->stride + 1) return ADVH_EINVAL;
    } else if (d->mode == ABL_FEATURE) {
        if (!d->mask || (d->mask_rows != 1 && d->mask_rows != d->B)) return ADVH_EINVAL;
    } else {
        return ADVH_EINVAL;
    }
    *c = AblCtx{d->x, d->base, d->mode == ABL_FEATURE ? d->mask : nullptr, (long)d->n, d->B, d->base_rows, d->mask_rows, d->mode,
                d->win, d->stride, d->K};
    return ADVH_OK;
}

extern "C" int advh_ablation_points(const advh_ablation_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    AblCtx c;
    if (ablation_ctx(d, &c) != ADVH_OK || !out || row0 < 0 || rows < 0) return ADVH_EINVAL;
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.base) && aligned16(out) && aligned16(c.mask);
    return build_rows(AblationRule{c}, vec, (long)row0, rows, out, (hipStream_t)stream);
}

extern "C" int advh_ablation_accumulate(const advh_ablation_desc* d, const float* f0, const float* fk, float* attr, advh_stream_t stream) {
    AblCtx c;
    if (ablation_ctx(d, &c) != ADVH_OK || !f0 || !fk || !attr) return ADVH_EINVAL;
    hipLaunchKernelGGL(ablation_accumulate_kernel, dim3(grid_for((long)c.B * c.n)), dim3(256), 0, (hipStream_t)stream, c, f0, fk, attr);
    return ADVH_LAUNCH_CHECK();
}
