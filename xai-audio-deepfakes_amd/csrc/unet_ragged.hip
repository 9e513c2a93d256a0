// Per-clip widths for the U-Net's maps (gfx950): the ragged forward runs the existing kernels over the batch's full width and
// clears, after every producer, what lies past each clip's own width -- a clip's columns then see the zeros its own zero
// padding would give, layer by layer.
//
// advh_fmap_clip_tail      the zero-haloed NHWC fp16 maps of gemm.FMap ([B][H + 2 PH][W + 2 PW][C]), single plane or split pair
// advh_zero_tail_cols_f32  the t-fastest fp32 planes [B][H][W] (mask, logits, the private copy of |X|)
//
// Both only store: no value past a clip's width is read, so NaN there costs nothing.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include "addvisor_hip.h"
#include "common.h"

namespace advh {
namespace unet_ragged {

__device__ __forceinline__ int clip_width(const int* __restrict__ widths, int b, int shift, int W) {
    const int w = widths[b] >> shift;
    return w < 0 ? 0 : w > W ? W : w;
}

// grid (1, H, B): one workgroup per interior row.  The tail of a row, columns [wb, W) x C channels, is one contiguous run of
// (W - wb) * C fp16 per plane: 16-byte stores.  ind >= 0: channel `ind` of every interior pixel is rewritten, (hi 1, lo 0)
// inside the clip's width and 0 past it (the run above covers the latter).
__global__ __launch_bounds__(256) void fmap_clip_tail_kernel(_Float16* __restrict__ x, long lo, const int* __restrict__ widths, int shift,
                                                             int H, int W, int C, int PH, int PW, int ind) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int wb = clip_width(widths, b, shift, W);
    _Float16* row = x + (((long)b * (H + 2 * PH) + y + PH) * (W + 2 * PW) + PW) * C;      // interior pixel (y, 0), channel 0
    const int chunks = (W - wb) * (C >> 3);
    int4* t = reinterpret_cast<int4*>(row + (long)wb * C);
    int4* tl = reinterpret_cast<int4*>(row + lo + (long)wb * C);
    const int4 z = make_int4(0, 0, 0, 0);
    for (int i = threadIdx.x; i < chunks; i += 256) {
        t[i] = z;
        if (lo) tl[i] = z;
    }
    if (ind >= 0)
        for (int xx = threadIdx.x; xx < wb; xx += 256) {
            row[(long)xx * C + ind] = (_Float16)1.0f;
            if (lo) row[lo + (long)xx * C + ind] = (_Float16)0.0f;
        }
}

// grid (ceil(H / 8), B): eight rows per workgroup, columns [wb, W) of each
__global__ __launch_bounds__(256) void zero_tail_cols_f32_kernel(float* __restrict__ x, const int* __restrict__ widths, int H, int W) {
    const int b = blockIdx.y, y0 = blockIdx.x * 8;
    const int wb = clip_width(widths, b, 0, W);
    const int tw = W - wb;
    if (tw <= 0) return;
    const int rows = min(8, H - y0);
    for (int i = threadIdx.x; i < rows * tw; i += 256) {
        const int r = i / tw, c = wb + i - r * tw;
        x[((long)b * H + y0 + r) * W + c] = 0.f;
    }
}

}  // namespace unet_ragged
}  // namespace advh

using namespace advh::unet_ragged;

extern "C" int advh_fmap_clip_tail(void* x, int64_t lo, const int32_t* widths, int shift, int B, int H, int W, int C, int PH, int PW,
                                   int ind_channel, advh_stream_t stream) {
    if (!x || !widths || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || PH < 0 || PW < 0 || shift < 0 || shift > 2) return ADVH_EINVAL;
    if (lo < 0 || lo % 8 || !aligned16(x) || ((uintptr_t)widths & 3) || ind_channel >= C) return ADVH_EINVAL;
    if (lo && lo < (int64_t)B * (H + 2 * PH) * (W + 2 * PW) * C) return ADVH_EINVAL;          // the planes may not overlap
    if (B > 65535 || H > 65535) return ADVH_EUNSUPPORTED;                                     // one workgroup per (clip, row)
    hipLaunchKernelGGL(fmap_clip_tail_kernel, dim3(1, H, B), dim3(256), 0, (hipStream_t)stream, (_Float16*)x, (long)lo, (const int*)widths,
                       shift, H, W, C, PH, PW, ind_channel < 0 ? -1 : ind_channel);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_zero_tail_cols_f32(float* x, const int32_t* widths, int B, int H, int W, advh_stream_t stream) {
    if (!x || !widths || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)x & 3) || ((uintptr_t)widths & 3)) return ADVH_EINVAL;
    if (B > 65535) return ADVH_EUNSUPPORTED;
    hipLaunchKernelGGL(zero_tail_cols_f32_kernel, dim3((H + 7) / 8, B), dim3(256), 0, (hipStream_t)stream, x, (const int*)widths, H, W);
    return ADVH_LAUNCH_CHECK();
}
