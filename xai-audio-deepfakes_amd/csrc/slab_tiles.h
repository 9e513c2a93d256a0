// The pieces that the slab-tiled row contractions share (concept.hip: the Gram kernel; influence.hip: the moment and
// squared-distance kernels): a problem is cut into 64 x 64 output blocks x slabs of the contraction, every slab's fp32 partial
// goes to a workspace [slab][M][N], and one fold launch adds the slabs in ascending order in fp64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace advh {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GR_BLK = 64;            // output block edge
constexpr int GR_KC = 64;             // floats of the contraction staged per step
constexpr int GR_PITCH = GR_KC + 4;   // LDS row pitch (floats): 16-byte aligned rows, 4-bank skew per row
constexpr int GR_SLAB_MIN = 512;      // shortest slab (floats)
constexpr long GR_TARGET_WG = 1024;   // workgroups aimed at: four per CU

struct GramPlan {
    long slab;      // floats per slab, a multiple of GR_KC
    int nslab;
    int bm, bn;     // blocks along M, N
    long nblk;      // blocks launched per slab
};

static GramPlan gram_plan(int M, int N, long F, int symmetric) {
    GramPlan p;
    p.bm = (M + GR_BLK - 1) / GR_BLK;
    p.bn = (N + GR_BLK - 1) / GR_BLK;
    p.nblk = symmetric ? (long)p.bm * (p.bm + 1) / 2 : (long)p.bm * p.bn;
    const long full = (long)p.bm * p.bn;                                 // the plan does not depend on the mode: one workspace size
    const long maxslabs = GR_TARGET_WG / full > 1 ? GR_TARGET_WG / full : 1;
    long slab = (F + maxslabs - 1) / maxslabs;
    slab = (slab + GR_KC - 1) / GR_KC * GR_KC;
    p.slab = slab < GR_SLAB_MIN ? GR_SLAB_MIN : slab;
    p.nslab = (int)((F + p.slab - 1) / p.slab);
    return p;
}

// rows [r0, r0 + ROWS) x columns [k0, k0 + COLS) of src (row stride ld) -> dst [ROWS][PITCH]; zero past `rows` and past `kend`.
// 256 threads; VEC = false stages with 4-byte loads alone.
template <bool VEC, int ROWS, int COLS, int PITCH>
__device__ __forceinline__ void stage_rows(float* dst, const float* __restrict__ src, long ld, int r0, int rows, long k0, long kend, int tid) {
#pragma unroll
    for (int q = 0; q < ROWS * COLS / 4 / 256; ++q) {
        const int i = q * 256 + tid, r = i / (COLS / 4), c = (i % (COLS / 4)) * 4;
        const long k = k0 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + r < rows && k < kend) {
            const float* p = src + (long)(r0 + r) * ld + k;
            if (VEC && k + 3 < kend) {
                v = *(const float4*)p;
            } else {
                v.x = p[0];
                if (k + 1 < kend) v.y = p[1];
                if (k + 2 < kend) v.z = p[2];
                if (k + 3 < kend) v.w = p[3];
            }
        }
        *(float4*)(dst + r * PITCH + c) = v;
    }
}

template <bool VEC>
__device__ __forceinline__ void gram_stage(float* dst, const float* __restrict__ src, long ld, int r0, int rows, long k0, long kend, int tid) {
    stage_rows<VEC, GR_BLK, GR_KC, GR_PITCH>(dst, src, ld, r0, rows, k0, kend, tid);
}

// blockIdx -> (bi, bj): symmetric mode counts the blocks bj >= bi row by row
__device__ __forceinline__ void block_of(int b, int bn, int symmetric, int& bi, int& bj) {
    if (symmetric) {
        int rest = b, row = 0;
        while (rest >= bn - row) { rest -= bn - row; ++row; }
        bi = row;
        bj = row + rest;
    } else {
        bi = b / bn;
        bj = b % bn;
    }
}

// G[i][j] = sum over slabs, ascending, in fp64.  Symmetric: the blocks below the diagonal were not computed, and every entry
// below the diagonal is read from its transpose.  (A template so that every translation unit may hold it.)
template <typename OUT>
__global__ __launch_bounds__(256) void gram_fold_kernel(const float* __restrict__ part, int M, int N, int nslab, int symmetric,
                                                        OUT* __restrict__ G) {
    const long total = (long)M * N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        long i = e / N, j = e - i * N;
        if (symmetric && i > j) { const long t = i; i = j; j = t; }
        const float* p = part + i * N + j;
        double s = 0.0;
        for (int q = 0; q < nslab; ++q) s += (double)p[(long)q * total];
        G[e] = s;
    }
}

}  // namespace advh
