// Entry points of the fp32-class 2-D line tile without the mask head; the kernel and its description are in conv_taps2d_x3.h.
#include "conv_taps2d_x3.h"

using namespace advh;

extern "C" int advh_conv_taps2d_split_lds_bytes(int C) {
    return C == 32 ? taps2d_x3_lds<32>() : (C == 64 ? taps2d_x3_lds<64>() : -1);
}

extern "C" int advh_conv_taps2d_split(const advh_taps2d_desc* d, int C, int64_t x_lo, int64_t w_lo, int64_t o_lo, advh_stream_t stream) {
    const int lds = advh_conv_taps2d_split_lds_bytes(C);
    long grid = 0;
    const int rc = advh_taps2d_split_check(d, C, x_lo, w_lo, o_lo, nullptr, lds, &grid);
    if (rc != ADVH_OK) return rc;
    const void* fn = C == 64 ? (const void*)conv_taps2d_x3_kernel<64, false> : (const void*)conv_taps2d_x3_kernel<32, false>;
    if (advh_ensure_lds(fn) != ADVH_OK) return ADVH_ELAUNCH;
    const taps2d_head none = {nullptr, 0.f, nullptr, nullptr};
    if (C == 64) hipLaunchKernelGGL((conv_taps2d_x3_kernel<64, false>), dim3((unsigned)grid), dim3(512), lds, (hipStream_t)stream, *d, (long)x_lo, (long)w_lo, (long)o_lo, none);
    else hipLaunchKernelGGL((conv_taps2d_x3_kernel<32, false>), dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, *d, (long)x_lo, (long)w_lo, (long)o_lo, none);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_conv_taps2d_x3)
