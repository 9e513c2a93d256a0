// Ablated batches and the attribution sums of the perturbation attributions (Captum's Occlusion and FeatureAblation):
// include/addvisor_hip.h, advh_ablation_points / advh_ablation_accumulate.
//
// Both kernels are memory-bound and tiny next to the K classifier forwards they serve (one forward row is on the order of a
// GFLOP; building it moves ~12 B per sample), so they stay simple: grid-stride loops, float4 access when every row pointer is
// 16-byte aligned (base pointers aligned and n % 4 == 0), a scalar path otherwise.
//
// Order contract: the Occlusion sum of sample (b, t) adds diff[k][b] for k = k_lo .. k_hi sequentially in increasing k from
// 0.f and divides by the count, as Captum's total_attrib += diff * mask; weights += mask; total_attrib / weights does (adding
// an exact zero for the windows that do not cover t changes nothing).  No prefix sums, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
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

// Which of the samples t .. t + N - 1 of ablated row (k, b) the baseline replaces (bit j: sample t + j); k < 0 is a padding
// row, a copy of x.  The N = 4 form reads the feature indices as one int4 (t % 4 == 0, mask row 16-byte aligned).
template <int N>
__device__ __forceinline__ unsigned ablated(const AblCtx& c, long k, const int32_t* mr, long t) {
    if (k < 0) return 0u;
    unsigned bits = 0u;
    if (c.mode == ABL_OCCLUSION) {
        const long lo = k * c.stride;
#pragma unroll
        for (int j = 0; j < N; ++j) bits |= (t + j >= lo && t + j < lo + c.win) ? 1u << j : 0u;
    } else if (N == 4) {
        const int4 m = *(const int4*)(mr + t);
        bits = (m.x == k ? 1u : 0u) | (m.y == k ? 2u : 0u) | (m.z == k ? 4u : 0u) | (m.w == k ? 8u : 0u);
    } else {
        bits = mr[t] == k ? 1u : 0u;
    }
    return bits;
}

// out[r][:] = ablated row g = row0 + r: base where sample t is in window / feature k = g / B, x[g % B] elsewhere
template <bool VEC>
__global__ __launch_bounds__(256) void ablation_points_kernel(AblCtx c, long row0, int rows, float* __restrict__ out) {
    const long per = VEC ? c.n / 4 : c.n, total = (long)rows * per, kb = (long)c.K * c.B;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per, g = row0 + r;
        const long b = g % c.B, k = g < kb ? g / c.B : -1L;
        const float* xr = c.x + b * c.n;
        const float* br = c.base + (c.base_rows == 1 ? 0L : b * c.n);
        const int32_t* mr = c.mode == ABL_FEATURE ? c.mask + (c.mask_rows == 1 ? 0L : b * c.n) : nullptr;
        if (VEC) {
            const long t = q * 4;
            const unsigned m = ablated<4>(c, k, mr, t);
            const float4 xv = *(const float4*)(xr + t), bv = *(const float4*)(br + t);
            *(float4*)(out + r * c.n + t) = make_float4(m & 1u ? bv.x : xv.x, m & 2u ? bv.y : xv.y, m & 4u ? bv.z : xv.z, m & 8u ? bv.w : xv.w);
        } else {
            out[r * c.n + q] = ablated<1>(c, k, mr, q) ? br[q] : xr[q];
        }
    }
}

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

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline unsigned grid_for(long work) {
    long blocks = (work + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > 8192 ? 8192 : blocks);
}

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
    if (rows == 0) return ADVH_OK;
    const bool vec = c.n % 4 == 0 && aligned16(c.x) && aligned16(c.base) && aligned16(out) && (!c.mask || aligned16(c.mask));
    const unsigned grid = grid_for((long)rows * (vec ? c.n / 4 : c.n));
    if (vec)
        hipLaunchKernelGGL(ablation_points_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, c, (long)row0, rows, out);
    else
        hipLaunchKernelGGL(ablation_points_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, c, (long)row0, rows, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_ablation_accumulate(const advh_ablation_desc* d, const float* f0, const float* fk, float* attr, advh_stream_t stream) {
    AblCtx c;
    if (ablation_ctx(d, &c) != ADVH_OK || !f0 || !fk || !attr) return ADVH_EINVAL;
    hipLaunchKernelGGL(ablation_accumulate_kernel, dim3(grid_for((long)c.B * c.n)), dim3(256), 0, (hipStream_t)stream, c, f0, fk, attr);
    return ADVH_LAUNCH_CHECK();
}
