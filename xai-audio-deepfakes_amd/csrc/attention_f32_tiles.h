// Operand helpers shared by the attention kernels that run on the fp32-input matrix instruction v_mfma_f32_16x16x4_f32
// (attention_bwd_f32.hip, attention_maps.hip, lrp.hip): the operands are split-format or plain fp16 matrices (lo == 0), joined to
// fp32 once, when staged into LDS or fetched into registers.  The operand layouts are described in attention_bwd_f32.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "device_math.h"

namespace advh {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float LOG2E = 1.4426950408889634f;         // softmax in the log2 domain: exp(x) = v_exp_f32(x log2 e)

#define MFMA4(acc, a4, b4)                                                        \
    do {                                                                          \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a4).x, (b4).x, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a4).y, (b4).y, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a4).z, (b4).z, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a4).w, (b4).w, acc, 0, 0, 0); \
    } while (0)

// four consecutive channels d .. d+3 of one row of a split-format / fp16 matrix (zeros past the real head dim)
__device__ __forceinline__ float4 grow4(const _Float16* base, long lo, long row_off, int d, int dm) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (d < dm) load_h_rt<4>(base, row_off + d, lo, v);
    return make_float4(v[0], v[1], v[2], v[3]);
}

// rows [0, T) x channels [0, dm) of a split-format / fp16 matrix (row stride ld) -> fp32 LDS tile [NKEY][D + 4], zero elsewhere
template <int NKEY, int D, int NTH>
__device__ __forceinline__ void stage_f32(float* dst, const _Float16* src, long lo, long ld, int T, int dm, int tid) {
    constexpr int PITCH = D + 4, CH = D / 8;
    for (int i = tid; i < NKEY * CH; i += NTH) {
        const int row = i / CH, c = i % CH;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < T && c * 8 < dm) load_h_rt<8>(src, (long)row * ld + c * 8, lo, v);
        *(float4*)(dst + row * PITCH + c * 8) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(dst + row * PITCH + c * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

}  // namespace advh
