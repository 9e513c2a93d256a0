// d1.block.3 of the fp32-class U-Net with the 1x1 mask head + sigmoid in its epilogue: the HEAD instantiation of the 32-channel
// 2-D line tile (conv_taps2d_x3.h, which describes it), in a translation unit of its own.
#include "conv_taps2d_x3.h"

using namespace advh;

extern "C" int advh_conv_taps2d_split_head(const advh_taps2d_desc* d, int C, int64_t x_lo, int64_t w_lo, const float* head_w, float head_b,
                                           float* mask, float* logits, advh_stream_t stream) {
    const taps2d_head hd = {head_w, head_b, mask, logits};
    const int lds = taps2d_x3_lds<32>();
    long grid = 0;
    const int rc = advh_taps2d_split_check(d, C, x_lo, w_lo, 0, &hd, lds, &grid);
    if (rc != ADVH_OK) return rc;
    if (advh_ensure_lds((const void*)conv_taps2d_x3_kernel<32, true>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((conv_taps2d_x3_kernel<32, true>), dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, *d, (long)x_lo, (long)w_lo, 0L, hd);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_conv_taps2d_head_x3)
