// Per-clip frame counts of a ragged batch, for the kernels that exist as `template <..., bool RAGGED>`: the batch instance
// (RAGGED = false) takes its bound from the T / L it is passed, the ragged one reads it per clip from an int32 vector that is the
// kernel's LAST argument, so the batch instance's argument offsets -- and with them its device code -- are those of a kernel that
// never had the argument.
#pragma once
#include <hip/hip_runtime.h>

namespace advh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// frames[b] clamped to [lo, Ts]: no content of `frames` moves an access out of clip b's Ts rows (or, for a vector of sample
// counts, out of its Ts samples; the waveform kernels pass lo = 10, one window of feature-encoder layer 0)
__device__ __forceinline__ int clip_frames(const int* __restrict__ frames, int b, int Ts, int lo = 1) {
    const int f = frames[b];
    return f < lo ? lo : (f > Ts ? Ts : f);
}

// rows [Tv, Ts) x this head's dm columns of dq | dk | dv (and of the lo plane when lo != 0) = 0
template <int NTH>
__device__ __forceinline__ void zero_tail(_Float16* dbase, long lo, long ld, int H, int Tv, int Ts, int dm, int tid) {
    const int ch = dm / 8, per = 3 * ch;
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < (Ts - Tv) * per; i += NTH) {
        const int row = Tv + i / per, j = i % per;
        _Float16* p = dbase + (long)row * ld + (long)(j / ch) * H + (j % ch) * 8;
        *(f16x8*)p = z;
        if (lo) *(f16x8*)(p + lo) = z;
    }
}

}  // namespace advh
