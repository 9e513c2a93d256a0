// Counter-based noise shared by the attribution kernels (attribution_paths.hip, attribution_metrics.hip): Philox4x32-10 keyed by
// the seed, counter (quad, row lo, row hi, 0); include/addvisor_hip.h, advh_philox_normal, states the scheme.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace advh {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): 10 rounds of two 32x32 -> 64 multiplies, Weyl key schedule.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

// (2 * (w >> 9) + 1) * 2^-24: an exact fp32 in (0, 1), symmetric about 1/2.
__device__ __forceinline__ float philox_uniform(uint32_t w) { return (float)(((w >> 9) << 1) | 1u) * 5.9604644775390625e-8f; }

// Four standard normals of (seed, row, quad): Box-Muller on the word pairs (x, y) and (z, w); cos/sin through sincospif of the
// exact 2u so the angle carries no rounding of 2*pi.
__device__ __forceinline__ float4 philox_normal4(uint64_t seed, long row, long quad) {
    const uint4 r = philox4x32_10(make_uint4((uint32_t)quad, (uint32_t)row, (uint32_t)((unsigned long)row >> 32), 0u),
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    const float ra = sqrtf(-2.f * logf(philox_uniform(r.x))), rb = sqrtf(-2.f * logf(philox_uniform(r.z)));
    float sa, ca, sb, cb;
    sincospif(2.f * philox_uniform(r.y), &sa, &ca);
    sincospif(2.f * philox_uniform(r.w), &sb, &cb);
    return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

}  // namespace advh
