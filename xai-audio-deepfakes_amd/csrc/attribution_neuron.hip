// Neuron attributions (captum.attr.Neuron*) on the encoder chain stopped at a layer in the forward and started there in the
// backward: include/addvisor_hip.h, advh_layer_seed / advh_neuron_values.  A neuron is a selection box over the [T][H] frame of
// hidden_states[l]: (t0, t1, tstep, h0, h1, hstep), half-open, positive steps; its value is the sum of the selected elements.
//
// As attribution_layer.hip the kernels are elementwise over fp32 rows: grid-stride loops over the element walkers of
// attribution_lanes.h, which states the float4 / scalar rule (float4 when base pointers are aligned and H % 4 == 0) and the row tree.
//
// Determinism contract: one thread per element; every product is rounded on its own (no FMA contraction); the box sum is the
// row tree in one workgroup per clip row.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_lanes.h"
#include "common.h"
#include "device_math.h"

namespace advh {

struct sel_box {
    int t0, t1, ts, h0, h1, hs;
};

__device__ __forceinline__ bool in_box(const sel_box& b, int t, int h) {
    return t >= b.t0 && t < b.t1 && (t - b.t0) % b.ts == 0 && h >= b.h0 && h < b.h1 && (h - b.h0) % b.hs == 0;
}

// The seed gradient at hidden_states[l]: element (r, t, h) of resid is scale * src (dense: src != NULL) or scale (* row_scale[r])
// inside the box and 0 elsewhere; op receives the fp16 copy (lo == 0) or the split pair of the same fp32 value (hi plane at op,
// lo plane `lo` elements behind; the checked conversion of device_math.h).  Every element of both outputs is written.
template <bool VEC>
__global__ __launch_bounds__(256) void layer_seed_kernel(const float* __restrict__ src, const float* __restrict__ row_scale, float scale,
                                                         int T, int H, sel_box box, float* __restrict__ resid, _Float16* __restrict__ op,
                                                         long lo, int split, long total) {
    constexpr int W = VEC ? 4 : 1;
    const long per = total / W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const long e = i * W;
        const long row = e / H;
        const int h = (int)(e - row * H), t = (int)(row % T);
        float in = 0.f;
        if (!src) in = row_scale ? __fmul_rn(scale, row_scale[row / T]) : scale;
        lanes<W> v;
        if (src) {
            const lanes<W> s = load_lanes<W>(src + e);
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = __fmul_rn(scale, s[j]);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = in_box(box, t, h + j) ? in : 0.f;
        }
        store_lanes<W>(resid + e, v);
        if (op) store_h_item<W>(op, e, split ? lo : 0L, v.v);
    }
}

// One workgroup per clip row, the row tree: out[r] = sum over the box of v[r][t][h].  The two forms walk different index sets, so
// this kernel keeps two loops: the float4 form walks the quads that cover [h0, h1) of every selected frame and masks the
// components outside the box, the scalar form walks the box's elements.
template <bool VEC>
__global__ __launch_bounds__(256) void neuron_values_kernel(const float* __restrict__ v, int T, int H, sel_box box, float* __restrict__ out) {
    const long r = blockIdx.x;
    const float* vr = v + r * (long)T * H;
    const int nt = (box.t1 - box.t0 + box.ts - 1) / box.ts;
    float s = 0.f;
    if (VEC) {
        const int q0 = box.h0 / 4, nq = (box.h1 + 3) / 4 - q0;
        for (long j = threadIdx.x; j < (long)nt * nq; j += 256) {
            const int t = box.t0 + (int)(j / nq) * box.ts, h = (q0 + (int)(j % nq)) * 4;
            const float4 a = *(const float4*)(vr + (long)t * H + h);
            const float x0 = in_box(box, t, h) ? a.x : 0.f, x1 = in_box(box, t, h + 1) ? a.y : 0.f;
            const float x2 = in_box(box, t, h + 2) ? a.z : 0.f, x3 = in_box(box, t, h + 3) ? a.w : 0.f;
            s += (x0 + x1) + (x2 + x3);
        }
    } else {
        const int nh = (box.h1 - box.h0 + box.hs - 1) / box.hs;
        for (long j = threadIdx.x; j < (long)nt * nh; j += 256) {
            const int t = box.t0 + (int)(j / nh) * box.ts, h = box.h0 + (int)(j % nh) * box.hs;
            s += vr[(long)t * H + h];
        }
    }
    s = block_sum(s);
    if (threadIdx.x == 0) out[r] = s;
}

}  // namespace advh

using namespace advh;

// a selection box inside [0, T) x [0, H): non-empty, positive steps
static inline bool box_ok(const int* b, int T, int H) {
    return b && b[0] >= 0 && b[0] < b[1] && b[1] <= T && b[2] > 0 && b[3] >= 0 && b[3] < b[4] && b[4] <= H && b[5] > 0;
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attribution_neuron)

extern "C" int advh_layer_seed(const float* src, const float* row_scale, float scale, int R, int T, int H, const int* box, float* resid,
                               void* op, int split, int64_t op_lo, advh_stream_t stream) {
    if (!resid || R <= 0 || T <= 0 || H <= 0 || !isfinite(scale) || (split != 0 && split != 1)) return ADVH_EINVAL;
    if (src ? row_scale != nullptr : !box_ok(box, T, H)) return ADVH_EINVAL;    // dense mode takes no row_scale, box mode needs a box
    const long total = (long)R * T * H;
    if (op && split && (op_lo < total || op_lo <= 0)) return ADVH_EINVAL;       // the lo plane may not overlap the hi plane
    sel_box b = {0, 1, 1, 0, 1, 1};
    if (!src) b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const bool vec = H % 4 == 0 && aligned16(src) && aligned16(resid) && (!op || (((uintptr_t)op & 7) == 0 && (!split || op_lo % 4 == 0)));
    const unsigned grid = grid_for(vec ? total / 4 : total);
    launch_vec(vec, layer_seed_kernel<true>, layer_seed_kernel<false>, dim3(grid), (hipStream_t)stream, src, row_scale, scale, T, H, b, resid,
               op, op_lo, split, total);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_neuron_values(const float* v, int R, int T, int H, const int* box, float* out, advh_stream_t stream) {
    if (!v || !out || R <= 0 || T <= 0 || H <= 0 || !box_ok(box, T, H)) return ADVH_EINVAL;
    const sel_box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    launch_vec(H % 4 == 0 && aligned16(v), neuron_values_kernel<true>, neuron_values_kernel<false>, dim3(R), (hipStream_t)stream, v, T, H, b, out);
    return ADVH_LAUNCH_CHECK();
}
