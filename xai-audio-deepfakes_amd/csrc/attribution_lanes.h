// The float4 / scalar rule and the row tree of the attribution kernels (attribution_paths / _metrics / _layer / _neuron /
// _robust.hip), stated once.  A kernel is `template <bool VEC>`: the entry point launches the float4 form when every row pointer
// is 16-byte aligned and the row length is a multiple of 4, the scalar form otherwise.  Both forms run ONE body, a
// `#pragma unroll` loop over the lanes of a pack; only the loads and stores below know which form they are in.  Nothing here
// does arithmetic except the tree's additions, so a file's `#pragma clang fp contract(off)` keeps covering all of its products.
//
// Two walking shapes, because the scalar forms' element-to-thread mapping is part of what the files promise:
//   element walkers (paths, layer, layer_seed): W = VEC ? 4 : 1, item i covers elements [i * W, i * W + W) -- one float4 or one
//     float per item.  load_lanes / store_lanes.
//   quad walkers (metrics, robust): both forms walk the quads q < (n + 3) / 4 of a row, thread t the quads t, t + 256, ... --
//     the float4 form with one float4 per quad, the scalar form with four guarded floats (4q + k < n, else `fill`), storing only
//     the lanes in range.  Lane k joins a row sum iff quad_lane<VEC>(q, k, n), so both forms add the same elements in the same
//     order and give the same bits.  load_quad / store_quad.
//
// The row tree: block_sum (block_reduce: the NaN-propagating maximum instead, for row_norm_kernel) of one value per thread of a 256-thread workgroup -- a wave64 __shfl_xor tree, then the
// four waves as (w0 + w1) + (w2 + w3).  Every thread returns the same bits (robust scales a whole row by them); a kernel that
// only has thread 0 write the result uses it there alone and the other threads' reads fall away.
#pragma once
#include <hip/hip_runtime.h>

namespace advh {

template <int W>
struct lanes {
    float v[W];
    __device__ __forceinline__ float& operator[](int k) { return v[k]; }
    __device__ __forceinline__ const float& operator[](int k) const { return v[k]; }
};

template <int W>
__device__ __forceinline__ lanes<W> fill_lanes(float f) {
    lanes<W> r;
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = f;
    return r;
}

// ---- element walkers: W elements at p
template <int W>
__device__ __forceinline__ lanes<W> load_lanes(const float* p) {
    static_assert(W == 4 || W == 1, "one float4 or one float");
    if constexpr (W == 4) {
        const float4 t = *(const float4*)p;
        return {{t.x, t.y, t.z, t.w}};
    } else {
        return {{*p}};
    }
}

template <int W>
__device__ __forceinline__ void store_lanes(float* p, const lanes<W>& r) {
    static_assert(W == 4 || W == 1, "one float4 or one float");
    if constexpr (W == 4)
        *(float4*)p = make_float4(r[0], r[1], r[2], r[3]);
    else
        *p = r[0];
}

// an optional row: W elements at p + off, or `fill` when p is absent
template <int W>
__device__ __forceinline__ lanes<W> load_lanes_or(const float* p, long off, float fill) {
    return p ? load_lanes<W>(p + off) : fill_lanes<W>(fill);
}

// ---- quad walkers: quad q of a row of n elements
template <bool VEC>
__device__ __forceinline__ bool quad_lane(long q, int k, long n) {
    return VEC || q * 4 + k < n;
}

template <bool VEC>
__device__ __forceinline__ lanes<4> load_quad(const float* row, long q, long n, float fill = 0.f) {
    if constexpr (VEC) {
        return load_lanes<4>(row + q * 4);
    } else {
        lanes<4> r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = q * 4 + k < n ? row[q * 4 + k] : fill;
        return r;
    }
}

template <bool VEC>
__device__ __forceinline__ lanes<4> load_quad_or(const float* row, long q, long n, float fill = 0.f) {
    return row ? load_quad<VEC>(row, q, n, fill) : fill_lanes<4>(fill);
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* row, long q, long n, const lanes<4>& r) {
    if constexpr (VEC) {
        store_lanes<4>(row + q * 4, r);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q * 4 + k < n) row[q * 4 + k] = r[k];
    }
}

// ---- the row tree
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ float block_reduce(float s, bool take_max) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(s, o, 64);
        s = take_max ? nanmax(s, t) : s + t;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return take_max ? nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_sum(float s) { return block_reduce(s, false); }

}  // namespace advh
