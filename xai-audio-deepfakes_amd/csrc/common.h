// Shared host-side helpers of libaddvisor_hip.
#pragma once
#include <hip/hip_runtime.h>
#include "addvisor_hip.h"

// Per-module one-time initialisation (dynamic-LDS attributes); defined in gemm.hip.
int advh_init_rest();
int advh_init_attention();   // attention.hip
int advh_init_attention_ragged();   // attention_ragged.hip
int advh_init_attention_long();   // attention_long.hip
int advh_init_stft_ragged();   // stft_ragged.hip: its own twiddle table and LDS limits
int advh_stft_ragged_set_fb(int fb);   // stft_ragged.hip follows advh_set_option("stft_frames_per_workgroup")
// per-translation-unit setters of the split-format range flag pointer (csrc/device_math.h: ADVH_SPLIT_FLAG_SETTER)
int advh_split_flag_attention(int* flag);
int advh_split_flag_attention_ragged(int* flag);
int advh_split_flag_attention_long(int* flag);
int advh_split_flag_attention_bwd_long(int* flag);   // attention_bwd_long.hip raises its LDS limits per launch (advh_ensure_lds): no init function
int advh_split_flag_attention_bwd_f32(int* flag);
int advh_split_flag_attribution_layer(int* flag);
int advh_split_flag_attribution_neuron(int* flag);
int advh_split_flag_attention_bwd_x3(int* flag);
int advh_split_flag_backward(int* flag);
int advh_split_flag_conv_taps(int* flag);
int advh_split_flag_frontend(int* flag);
int advh_split_flag_frontend_bwd(int* flag);
int advh_split_flag_gemm(int* flag);
int advh_split_flag_hifigan(int* flag);
int advh_split_flag_rowops(int* flag);
int advh_split_flag_unet_misc(int* flag);
int advh_split_flag_unet_train(int* flag);
int advh_split_flag_resblock_pair_x3(int* flag);
int advh_split_flag_conv_taps2d_x3(int* flag);
int advh_split_flag_conv_taps2d_head_x3(int* flag);
int advh_split_flag_upconv_tile_x3(int* flag);
int advh_split_flag_conv_s21_tile_x3(int* flag);
int advh_split_flag_lrp(int* flag);
int advh_split_flag_attention_maps_long(int* flag);   // attention_maps_long.hip: advh_ensure_lds per launch, no init function

// attention backward of the fp32-class mode: the split-arithmetic kernel for head dims <= 64 (attention_bwd_x3.hip), called by
// advh_attention_bwd_split / _split_ragged (attention_bwd_f32.hip) after they validated the arguments; frames != nullptr: the ragged
// instances; g_att_bwd_force_f32: advh_set_option("attention_bwd_mfma_f32")
int advh_attention_bwd_x3_launch(const void* qkv, long qkv_lo, const void* dctx, long dctx_lo, void* dqkv, long dqkv_lo, const int* frames,
                                 int B, int T, int H, int heads, hipStream_t s);
extern int g_att_bwd_force_f32;

// Raise a kernel's dynamic-LDS limit to `bytes` once per (kernel, DEVICE): the attribute belongs to the device's copy of
// the code object, and one process may drive several GPUs (a per-process "done" flag left the second device at 64 KiB).
#include <mutex>
#include <set>
#include <utility>
inline int advh_ensure_lds(const void* fn, int bytes = 160 * 1024) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ADVH_ELAUNCH;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, dev})) return ADVH_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return ADVH_ELAUNCH;
    done.insert({fn, dev});
    return ADVH_OK;
}

#define ADVH_LAUNCH_CHECK() (hipGetLastError() == hipSuccess ? ADVH_OK : ADVH_ELAUNCH)

// The precondition of a float4 / int4 access through p.  nullptr (an optional pointer that is absent) passes.
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Blocks of 256 threads for a grid-stride loop over `work` items: at least one, at most `cap`.
inline unsigned grid_for(long work, long cap = 8192) {
    const long blocks = (work + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

// One launch of a kernel that exists in a float4 and a scalar form (`template <bool VEC>`): `vec`, the entry point's own
// alignment predicate, picks the instantiation.  256 threads, no dynamic LDS; the arguments convert to the kernel's parameter types.
template <class... P, class... A>
inline void launch_vec(bool vec, void (*kvec)(P...), void (*kscalar)(P...), dim3 grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(vec ? kvec : kscalar, grid, dim3(256), 0, s, static_cast<P>(args)...);
}
