// Layer attributions (captum.attr.Layer*, InternalInfluence) on the encoder chain started and stopped at a layer:
// include/addvisor_hip.h, advh_layer_inject / advh_layer_tap / advh_layer_conductance_accumulate.  The activation-space path of
// LayerIntegratedGradients and the weighted gradient sums reuse advh_attr_path_points / advh_attr_path_accumulate
// (csrc/attribution_paths.hip) with n = T * H.
//
// Every kernel here is elementwise over fp32 rows (a [B * T][H] residual buffer next to the layers' GEMMs), so they stay simple,
// as attribution_paths.hip: grid-stride loops, float4 access when every row pointer is 16-byte aligned (base pointers aligned and
// n % 4 == 0), a scalar path otherwise.
//
// Determinism contract: one thread per element; every product, difference and sum is rounded on its own (no FMA contraction), and
// the conductance sum adds its pairs in increasing step order with the pair that straddles a chunk boundary carried in
// [B][n] buffers, so the arithmetic of an element is the same sequence for every chunking.  Row sums are a fixed-shape tree in one
// workgroup.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"

namespace advh {

// resid[i] = src[i]; op[i] = fp16(src[i]) (lo == 0) or the split pair (hi plane at op, lo plane `lo` elements behind), from the
// same fp32 value.  The split conversion is the checked one (device_math.h): |x| > 65504 saturates and raises the range flag,
// NaN stays NaN planes.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_inject_kernel(const float* __restrict__ src, float* __restrict__ resid,
                                                           _Float16* __restrict__ op, long lo, int split, long total) {
    const long per = VEC ? total / 4 : total;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        if (VEC) {
            const float4 t = *(const float4*)(src + i * 4);
            *(float4*)(resid + i * 4) = t;
            if (op) {
                const float v[4] = {t.x, t.y, t.z, t.w};
                store_h_rt<4>(op, i * 4, split ? lo : 0L, v);
            }
        } else {
            const float t = src[i];
            resid[i] = t;
            if (op) {
                if (split) {
                    _Float16 h, l;
                    split_f32(t, h, l);
                    op[i] = h;
                    op[i + lo] = l;
                } else {
                    op[i] = (_Float16)t;
                }
            }
        }
    }
}

// out = g * inv_scale (* act): each product rounded on its own
template <bool VEC>
__global__ __launch_bounds__(256) void layer_tap_kernel(const float* __restrict__ g, const float* __restrict__ act, float inv_scale,
                                                        long total, float* __restrict__ out) {
    const long per = VEC ? total / 4 : total;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        if (VEC) {
            const float4 t = *(const float4*)(g + i * 4);
            float4 o = make_float4(__fmul_rn(t.x, inv_scale), __fmul_rn(t.y, inv_scale), __fmul_rn(t.z, inv_scale), __fmul_rn(t.w, inv_scale));
            if (act) {
                const float4 a = *(const float4*)(act + i * 4);
                o = make_float4(__fmul_rn(o.x, a.x), __fmul_rn(o.y, a.y), __fmul_rn(o.z, a.z), __fmul_rn(o.w, a.w));
            }
            *(float4*)(out + i * 4) = o;
        } else {
            float o = __fmul_rn(g[i], inv_scale);
            if (act) o = __fmul_rn(o, act[i]);
            out[i] = o;
        }
    }
}

// One workgroup per row, fixed-shape tree: sum[r] = sum_j g * inv_scale (* act), the values advh_layer_tap writes.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_tap_row_sum_kernel(const float* __restrict__ g, const float* __restrict__ act, float inv_scale,
                                                                long n, float* __restrict__ sum) {
    __shared__ float red[4];
    const long r = blockIdx.x;
    const float* gr = g + r * n;
    const float* ar = act ? act + r * n : nullptr;
    float s = 0.f;
    if (VEC) {
        for (long q = threadIdx.x; q < n / 4; q += 256) {
            const float4 t = *(const float4*)(gr + q * 4);
            float4 o = make_float4(__fmul_rn(t.x, inv_scale), __fmul_rn(t.y, inv_scale), __fmul_rn(t.z, inv_scale), __fmul_rn(t.w, inv_scale));
            if (ar) {
                const float4 a = *(const float4*)(ar + q * 4);
                o = make_float4(__fmul_rn(o.x, a.x), __fmul_rn(o.y, a.y), __fmul_rn(o.z, a.z), __fmul_rn(o.w, a.w));
            }
            s += (o.x + o.y) + (o.z + o.w);
        }
    } else {
        for (long j = threadIdx.x; j < n; j += 256) {
            float o = __fmul_rn(gr[j], inv_scale);
            if (ar) o = __fmul_rn(o, ar[j]);
            s += o;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sum[r] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float cond_term(float pg, float a, float pa) { return __fmul_rn(pg, __fsub_rn(a, pa)); }

// Conductance, one step-major chunk: element (b, j) walks the chunk's steps k = 0 .. steps - 1 in order,
//   total += pg * (act[k] - pa)   (skipped for the very first point: `first` and k == 0)
//   pa = act[k];  pg = grad[k] (k < ngrad)
// with (pg, pa) read from and written back to the carried pair, so a pair whose points lie in two chunks is the same product.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_conductance_kernel(const float* __restrict__ grad, const float* __restrict__ act, int B, long n,
                                                                int steps, int ngrad, int first, float* __restrict__ prev_grad,
                                                                float* __restrict__ prev_act, float* __restrict__ tot) {
    const long per = VEC ? n / 4 : n, total = (long)B * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / per, q = i - b * per;
        if (VEC) {
            const long e = b * n + q * 4;
            float4 acc = *(const float4*)(tot + e);
            float4 pg = make_float4(0.f, 0.f, 0.f, 0.f), pa = pg;
            if (!first) pg = *(const float4*)(prev_grad + e), pa = *(const float4*)(prev_act + e);
            for (int k = 0; k < steps; ++k) {
                const long o = ((long)k * B + b) * n + q * 4;
                const float4 a = *(const float4*)(act + o);
                if (!(first && k == 0)) {
                    acc.x = __fadd_rn(acc.x, cond_term(pg.x, a.x, pa.x)), acc.y = __fadd_rn(acc.y, cond_term(pg.y, a.y, pa.y));
                    acc.z = __fadd_rn(acc.z, cond_term(pg.z, a.z, pa.z)), acc.w = __fadd_rn(acc.w, cond_term(pg.w, a.w, pa.w));
                }
                pa = a;
                if (k < ngrad) pg = *(const float4*)(grad + o);
            }
            *(float4*)(tot + e) = acc;
            *(float4*)(prev_grad + e) = pg;
            *(float4*)(prev_act + e) = pa;
        } else {
            const long e = b * n + q;
            float acc = tot[e], pg = 0.f, pa = 0.f;
            if (!first) pg = prev_grad[e], pa = prev_act[e];
            for (int k = 0; k < steps; ++k) {
                const long o = ((long)k * B + b) * n + q;
                const float a = act[o];
                if (!(first && k == 0)) acc = __fadd_rn(acc, cond_term(pg, a, pa));
                pa = a;
                if (k < ngrad) pg = grad[o];
            }
            tot[e] = acc;
            prev_grad[e] = pg;
            prev_act[e] = pa;
        }
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
    if (vec)
        hipLaunchKernelGGL(layer_inject_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, resid, (_Float16*)op, (long)op_lo,
                           split, total);
    else
        hipLaunchKernelGGL(layer_inject_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, resid, (_Float16*)op, (long)op_lo,
                           split, total);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_layer_tap(const float* g, const float* act, float inv_scale, int rows, int64_t n, float* out, float* row_sum,
                              advh_stream_t stream) {
    if (!g || (!out && !row_sum) || rows <= 0 || n <= 0 || !isfinite(inv_scale)) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && aligned16(g) && aligned16(act) && aligned16(out);
    const long total = (long)rows * n;
    if (out) {
        if (vec)
            hipLaunchKernelGGL(layer_tap_kernel<true>, dim3(grid_for(total / 4)), dim3(256), 0, s, g, act, inv_scale, total, out);
        else
            hipLaunchKernelGGL(layer_tap_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, g, act, inv_scale, total, out);
    }
    if (row_sum) {
        if (vec)
            hipLaunchKernelGGL(layer_tap_row_sum_kernel<true>, dim3(rows), dim3(256), 0, s, g, act, inv_scale, (long)n, row_sum);
        else
            hipLaunchKernelGGL(layer_tap_row_sum_kernel<false>, dim3(rows), dim3(256), 0, s, g, act, inv_scale, (long)n, row_sum);
    }
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_layer_conductance_accumulate(const float* grad, const float* act, int B, int64_t n, int steps, int ngrad, int first,
                                                 float* prev_grad, float* prev_act, float* total, advh_stream_t stream) {
    if (!act || !prev_grad || !prev_act || !total || B <= 0 || n <= 0 || steps <= 0 || ngrad < 0 || ngrad > steps || (ngrad > 0 && !grad) ||
        (first != 0 && first != 1))
        return ADVH_EINVAL;
    const bool vec = n % 4 == 0 && aligned16(grad) && aligned16(act) && aligned16(prev_grad) && aligned16(prev_act) && aligned16(total);
    const unsigned grid = grid_for((long)B * (vec ? n / 4 : n));
    if (vec)
        hipLaunchKernelGGL(layer_conductance_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad, act, B, (long)n, steps, ngrad,
                           first, prev_grad, prev_act, total);
    else
        hipLaunchKernelGGL(layer_conductance_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad, act, B, (long)n, steps, ngrad,
                           first, prev_grad, prev_act, total);
    return ADVH_LAUNCH_CHECK();
}
