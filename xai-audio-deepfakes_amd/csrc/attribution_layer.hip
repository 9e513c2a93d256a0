// Layer attributions (captum.attr.Layer*, InternalInfluence) on the encoder chain started and stopped at a layer:
// include/addvisor_hip.h, advh_layer_inject / advh_layer_tap / advh_layer_conductance_accumulate.  The activation-space path of
// LayerIntegratedGradients and the weighted gradient sums reuse advh_attr_path_points / advh_attr_path_accumulate
// (csrc/attribution_paths.hip) with n = T * H.
//
// Every kernel here is elementwise over fp32 rows (a [B * T][H] residual buffer next to the layers' GEMMs), so they stay simple,
// as attribution_paths.hip: grid-stride loops over the element walkers of attribution_lanes.h, which states the float4 / scalar
// rule (float4 when base pointers are aligned and n % 4 == 0) and the row tree.
//
// Determinism contract: one thread per element; every product of the tap is rounded on its own, the conductance sum is one
// fused multiply-add per pair, and it adds its pairs in increasing step order with the pair that straddles a chunk boundary carried in
// [B][n] buffers, so the arithmetic of an element is the same sequence for every chunking.  Row sums are the row tree in one
// workgroup.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"
#include "device_math.h"

namespace advh {

// resid[i] = src[i]; op[i] = fp16(src[i]) (lo == 0) or the split pair (hi plane at op, lo plane `lo` elements behind), from the
// same fp32 value.  The split conversion is the checked one (device_math.h): |x| > 65504 saturates and raises the range flag,
// NaN stays NaN planes.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_inject_kernel(const float* __restrict__ src, float* __restrict__ resid,
                                                           _Float16* __restrict__ op, long lo, int split, long total) {
    constexpr int W = VEC ? 4 : 1;
    const long per = total / W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const lanes<W> t = load_lanes<W>(src + i * W);
        store_lanes<W>(resid + i * W, t);
        if (op) store_h_item<W>(op, i * W, split ? lo : 0L, t.v);
    }
}

// W elements of g * inv_scale (* act) at offset e: each product rounded on its own
template <int W>
__device__ __forceinline__ lanes<W> tap_lanes(const float* g, const float* act, float inv_scale, long e) {
    lanes<W> o = load_lanes<W>(g + e);
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = __fmul_rn(o[k], inv_scale);
    if (act) {
        const lanes<W> a = load_lanes<W>(act + e);
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = __fmul_rn(o[k], a[k]);
    }
    return o;
}

// out = g * inv_scale (* act)
template <bool VEC>
__global__ __launch_bounds__(256) void layer_tap_kernel(const float* __restrict__ g, const float* __restrict__ act, float inv_scale,
                                                        long total, float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const long per = total / W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256)
        store_lanes<W>(out + i * W, tap_lanes<W>(g, act, inv_scale, i * W));
}

// One workgroup per row, the row tree: sum[r] = sum_j g * inv_scale (* act), the values advh_layer_tap writes.  A thread adds
// one value per element in the scalar form and (x0 + x1) + (x2 + x3) per quad in the float4 form.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_tap_row_sum_kernel(const float* __restrict__ g, const float* __restrict__ act, float inv_scale,
                                                                long n, float* __restrict__ sum) {
    constexpr int W = VEC ? 4 : 1;
    const long r = blockIdx.x;
    const float* gr = g + r * n;
    const float* ar = act ? act + r * n : nullptr;
    float s = 0.f;
    for (long q = threadIdx.x; q < n / W; q += 256) {
        const lanes<W> o = tap_lanes<W>(gr, ar, inv_scale, q * W);
        if constexpr (W == 4)
            s += (o[0] + o[1]) + (o[2] + o[3]);
        else
            s += o[0];
    }
    s = block_sum(s);
    if (threadIdx.x == 0) sum[r] = s;
}

// Conductance, one step-major chunk: element (b, j) walks the chunk's steps k = 0 .. steps - 1 in order,
//   total = fma(pg, act[k] - pa, total)   (skipped for the very first point: `first` and k == 0; the difference is rounded, the
//                                          product joins the sum unrounded -- what the compiler made of the former
//                                          __fadd_rn(total, __fmul_rn(pg, .)), plain operators in this toolchain, now stated)
//   pa = act[k];  pg = grad[k] (k < ngrad)
// with (pg, pa) read from and written back to the carried pair, so a pair whose points lie in two chunks is the same product.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_conductance_kernel(const float* __restrict__ grad, const float* __restrict__ act, int B, long n,
                                                                int steps, int ngrad, int first, float* __restrict__ prev_grad,
                                                                float* __restrict__ prev_act, float* __restrict__ tot) {
    constexpr int W = VEC ? 4 : 1;
    const long per = n / W, total = (long)B * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / per, q = i - b * per;
        const long e = b * n + q * W;
        lanes<W> acc = load_lanes<W>(tot + e), pg = fill_lanes<W>(0.f), pa = pg;
        if (!first) pg = load_lanes<W>(prev_grad + e), pa = load_lanes<W>(prev_act + e);
        for (int k = 0; k < steps; ++k) {
            const long o = ((long)k * B + b) * n + q * W;
            const lanes<W> a = load_lanes<W>(act + o);
            if (!(first && k == 0)) {
#pragma unroll
                for (int l = 0; l < W; ++l) acc[l] = fmaf(pg[l], a[l] - pa[l], acc[l]);
            }
            pa = a;
            if (k < ngrad) pg = load_lanes<W>(grad + o);
        }
        store_lanes<W>(tot + e, acc);
        store_lanes<W>(prev_grad + e, pg);
        store_lanes<W>(prev_act + e, pa);
    }
}

}  // namespace advh

using namespace advh;

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attribution_layer)

extern "C" int advh_layer_inject(const float* src, int rows, int64_t n, float* resid, void* op, int split, int64_t op_lo,
                                 advh_stream_t stream) {
    if (!src || !resid || rows <= 0 || n <= 0 || (split != 0 && split != 1)) return ADVH_EINVAL;
    const long total = (long)rows * n;
    if (op && split && (op_lo < total || op_lo <= 0)) return ADVH_EINVAL;       // the lo plane may not overlap the hi plane
    const bool vec = n % 4 == 0 && aligned16(src) && aligned16(resid) && (!op || (((uintptr_t)op & 7) == 0 && (!split || op_lo % 4 == 0)));
    const unsigned grid = grid_for(vec ? total / 4 : total);
    launch_vec(vec, layer_inject_kernel<true>, layer_inject_kernel<false>, dim3(grid), (hipStream_t)stream, src, resid, op, op_lo, split, total);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_layer_tap(const float* g, const float* act, float inv_scale, int rows, int64_t n, float* out, float* row_sum,
                              advh_stream_t stream) {
    if (!g || (!out && !row_sum) || rows <= 0 || n <= 0 || !isfinite(inv_scale)) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && aligned16(g) && aligned16(act) && aligned16(out);
    const long total = (long)rows * n;
    if (out)
        launch_vec(vec, layer_tap_kernel<true>, layer_tap_kernel<false>, dim3(grid_for(vec ? total / 4 : total)), s, g, act, inv_scale, total, out);
    if (row_sum)
        launch_vec(vec, layer_tap_row_sum_kernel<true>, layer_tap_row_sum_kernel<false>, dim3(rows), s, g, act, inv_scale, n, row_sum);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_layer_conductance_accumulate(const float* grad, const float* act, int B, int64_t n, int steps, int ngrad, int first,
                                                 float* prev_grad, float* prev_act, float* total, advh_stream_t stream) {
    if (!act || !prev_grad || !prev_act || !total || B <= 0 || n <= 0 || steps <= 0 || ngrad < 0 || ngrad > steps || (ngrad > 0 && !grad) ||
        (first != 0 && first != 1))
        return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(grad) && aligned16(act) && aligned16(prev_grad) && aligned16(prev_act) && aligned16(total);
    const unsigned grid = grid_for((long)B * (vec ? n / 4 : n));
    launch_vec(vec, layer_conductance_kernel<true>, layer_conductance_kernel<false>, dim3(grid), (hipStream_t)stream, grad, act, B, n, steps,
               ngrad, first, prev_grad, prev_act, total);
    return ADVH_LAUNCH_CHECK();
}
