// Concept activation vectors (TCAV, Kim et al. 2018) on long flattened activations: include/addvisor_hip.h,
// advh_concept_gram / advh_concept_gram_workspace / advh_concept_combine / advh_concept_time_pool.
//
// A concept example is one row of F = T * H floats (152 832 at wav2vec2-base, 4 s) and there are N << F of them, so the fit of a
// linear concept classifier needs only the N x N Gram matrix; the CAV is then w = X^T a, and a TCAV score is one more row
// product <grad, w>.  All three are long contractions over rows that already sit in HBM:
//
//   gram      : G[i][j] = sum_f X[i][f] * Y[j][f]      (NT form: both operands contiguous along f), double out
//   combine   : W[c][f] = sum_i A[c][i] * X[i][f]      (the CAV from the dual coefficients)
//   time_pool : out[r][h] = sum_t X[r][t][h] (* 1/T)
//
// Everything is bit-identical from run to run: no atomics, one fixed summation order.
//
// gram.  F is cut into slabs (a multiple of GR_KC floats, at least GR_SLAB_MIN: gram_plan) so that a 128 x 128 problem still
// gives several hundred workgroups.  One workgroup = one 64 x 64 output block x one slab, four wavefronts, each owning a 32 x 32
// quarter as 2 x 2 tiles of v_mfma_f32_16x16x4_f32 (four independent accumulators per wave).  The slab is walked GR_KC = 64
// floats at a time: 64 rows of X and 64 rows of Y go through LDS as fp32 [64][GR_KC + 4] with 16-byte global loads; a lane
// reads one float4 of its A row and one of its B row at k = 4 (lane / 16) and feeds four MFMAs with .x .y .z .w -- the k order
// inside a step is permuted, identically for both operands.  The f32 MFMA is a k-ordered fmaf chain, so a partial is one fixed
// chain per output.  Rows past M / N and columns past the slab's end are staged as zeros (they add +0 to a chain), so no tail
// needs a padded copy.  The fp32 partial goes to part[slab][M][N]; gram_fold_kernel adds the slabs in ascending order in fp64.
// Symmetric mode: only blocks with bj >= bi are launched, and the fold reads entry (i, j), i > j, from (j, i): the mirrored
// entries are the same bits by construction.  A base pointer or stride that is not 16-byte aligned takes the VEC = false
// instance, which stages with 4-byte loads alone (a misaligned 16-byte load is never issued).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "addvisor_hip.h"
#include "common.h"
#include "slab_tiles.h"   // the staging, the slab plan and the fold, shared with influence.hip

namespace advh {

template <bool VEC>
__global__ __launch_bounds__(256) void gram_partial_kernel(const float* __restrict__ X, long ldx, const float* __restrict__ Y, long ldy, int M,
                                                           int N, long F, long slab, int bn, int symmetric, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Xs[GR_BLK * GR_PITCH];
    __shared__ __attribute__((aligned(16))) float Ys[GR_BLK * GR_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    int bi, bj;
    block_of((int)blockIdx.x, bn, symmetric, bi, bj);
    const int i0 = bi * GR_BLK, j0 = bj * GR_BLK;
    const long kbeg = (long)blockIdx.y * slab, kend = kbeg + slab < F ? kbeg + slab : F;
    const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;                   // this wavefront's quarter of the block

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long k0 = kbeg; k0 < kend; k0 += GR_KC) {
        if (k0 != kbeg) __syncthreads();                                 // the previous step's tiles are no longer read
        gram_stage<VEC>(Xs, X, ldx, i0, M, k0, kend, tid);
        gram_stage<VEC>(Ys, Y, ldy, j0, N, k0, kend, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GR_KC; kk += 16) {
            float4 af[2], bf[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = *(const float4*)(Xs + (wi + a * 16 + fr) * GR_PITCH + kk + 4 * g);
#pragma unroll
            for (int b = 0; b < 2; ++b) bf[b] = *(const float4*)(Ys + (wj + b * 16 + fr) * GR_PITCH + kk + 4 * g);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a].x, bf[b].x, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a].y, bf[b].y, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a].z, bf[b].z, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a].w, bf[b].w, acc[a][b], 0, 0, 0);
                }
        }
    }
    // accumulator layout of the 16 x 16 tile: column (j) = lane % 16, row (i) = 4 (lane / 16) + register
    float* ps = part + (long)blockIdx.y * M * N;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = j0 + wj + b * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wi + a * 16 + 4 * g + r;
                if (i < M && j < N) ps[(long)i * N + j] = acc[a][b][r];
            }
        }
}

// W[c][f] = fmaf chain over i ascending, from 0.f; one thread owns VW consecutive f of up to CB rows c: X is read once per
// group of CB coefficient rows.  A[c][i] is wave-uniform.
constexpr int CB = 8;

template <int VW>
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ A, const float* __restrict__ X, long ldx, int c0, int nc, int N,
                                                      long F, float* __restrict__ W, long ldw) {
    const long per = (F + VW - 1) / VW;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < per; q += (long)gridDim.x * 256) {
        const long f = q * VW;
        float acc[CB][VW];
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int v = 0; v < VW; ++v) acc[c][v] = 0.f;
        for (int i = 0; i < N; ++i) {
            float x[VW];
            if (VW == 4) {
                const float4 t = *(const float4*)(X + (long)i * ldx + f);
                x[0] = t.x; x[1 % VW] = t.y; x[2 % VW] = t.z; x[3 % VW] = t.w;
            } else {
                x[0] = X[(long)i * ldx + f];
            }
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                if (c < nc) {
                    const float a = A[(long)(c0 + c) * N + i];
#pragma unroll
                    for (int v = 0; v < VW; ++v) acc[c][v] = fmaf(a, x[v], acc[c][v]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            if (c < nc) {
                float* w = W + (long)(c0 + c) * ldw + f;
                if (VW == 4) *(float4*)w = make_float4(acc[c][0], acc[c][1 % VW], acc[c][2 % VW], acc[c][3 % VW]);
                else w[0] = acc[c][0];
            }
        }
    }
}

// out[r][h] = sum over t ascending of X[r][t][h], from 0.f; mode 1: times inv_t
__global__ __launch_bounds__(256) void time_pool_kernel(const float* __restrict__ X, long R, int T, int H, int mode, float inv_t,
                                                        float* __restrict__ out) {
    const long total = R * H;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / H, h = e - r * H;
        const float* p = X + r * T * H + h;
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += p[(long)t * H];
        out[e] = mode ? s * inv_t : s;
    }
}

}  // namespace advh

using namespace advh;

constexpr long GRID_CAP = 16384;   // blocks of the grid-stride kernels (twice common.h's default)

static bool gram_args_ok(int M, int N, int64_t F) { return M > 0 && N > 0 && F > 0 && M <= (1 << 20) && N <= (1 << 20) && F <= (1LL << 40); }

extern "C" int64_t advh_concept_gram_workspace(int M, int N, int64_t F) {
    if (!gram_args_ok(M, N, F)) return ADVH_EINVAL;
    return (int64_t)gram_plan(M, N, (long)F, 0).nslab * M * N * (int64_t)sizeof(float);
}

extern "C" int advh_concept_gram(const float* X, int64_t ldx, const float* Y, int64_t ldy, int M, int N, int64_t F, int symmetric, float* workspace,
                                 double* G, advh_stream_t stream) {
    if (!X || !Y || !workspace || !G || !gram_args_ok(M, N, F) || ldx < F || ldy < F) return ADVH_EINVAL;
    if (symmetric != 0 && symmetric != 1) return ADVH_EINVAL;
    if (symmetric && (Y != X || M != N || ldy != ldx)) return ADVH_EINVAL;
    if (((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)G & 7)) return ADVH_EINVAL;
    const GramPlan p = gram_plan(M, N, (long)F, symmetric);
    if (p.nblk > 0x7fffffffL || p.nslab > 65535) return ADVH_EUNSUPPORTED;
    const bool vec = aligned16(X) && aligned16(Y) && ldx % 4 == 0 && ldy % 4 == 0;
    const dim3 grid((unsigned)p.nblk, (unsigned)p.nslab);
    hipStream_t s = (hipStream_t)stream;
    launch_vec(vec, gram_partial_kernel<true>, gram_partial_kernel<false>, grid, s, X, ldx, Y, ldy, M, N, F, p.slab, p.bn, symmetric, workspace);
    if (ADVH_LAUNCH_CHECK() != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL(gram_fold_kernel<double>, dim3(grid_for((long)M * N, GRID_CAP)), dim3(256), 0, s, workspace, M, N, p.nslab, symmetric, G);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_concept_combine(const float* A, const float* X, int64_t ldx, int C, int N, int64_t F, float* W, int64_t ldw,
                                    advh_stream_t stream) {
    if (!A || !X || !W || C <= 0 || N <= 0 || F <= 0 || ldx < F || ldw < F || F > (1LL << 40)) return ADVH_EINVAL;
    if (((uintptr_t)A & 3) || ((uintptr_t)X & 3) || ((uintptr_t)W & 3)) return ADVH_EINVAL;
    const bool vec = aligned16(X) && aligned16(W) && ldx % 4 == 0 && ldw % 4 == 0 && F % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    for (int c0 = 0; c0 < C; c0 += CB) {
        const int nc = C - c0 < CB ? C - c0 : CB;
        launch_vec(vec, combine_kernel<4>, combine_kernel<1>, dim3(grid_for(vec ? (long)F / 4 : (long)F, GRID_CAP)), s, A, X, ldx, c0, nc, N, F, W, ldw);
        if (ADVH_LAUNCH_CHECK() != ADVH_OK) return ADVH_ELAUNCH;
    }
    return ADVH_OK;
}

extern "C" int advh_concept_time_pool(const float* X, int64_t R, int T, int H, int mode, float* out, advh_stream_t stream) {
    if (!X || !out || R <= 0 || T <= 0 || H <= 0 || (mode != 0 && mode != 1) || R > (1LL << 40)) return ADVH_EINVAL;
    const float inv_t = (float)(1.0 / (double)T);
    hipLaunchKernelGGL(time_pool_kernel, dim3(grid_for((long)R * H, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, X, (long)R, T, H, mode, inv_t, out);
    return ADVH_LAUNCH_CHECK();
}
