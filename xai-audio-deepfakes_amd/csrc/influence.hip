// Training-data influence (captum.influence: SimilarityInfluence, TracInCPFast; influence functions, Koh & Liang 2017) on rows that
// already sit in HBM: include/addvisor_hip.h, advh_influence_*.
//
//   moment   : Hm[f][g] = sum_i w[i] X[i][f] X[i][g]     (the logistic Hessian's data term; contraction over the ROWS), double out
//   sqdist   : D[i][j]  = sum_f (X[i][f] - Y[j][f])^2    (direct differences: a + b - 2G cancels for near-duplicates), double out
//   sumsq    : out[i]   = sum_f X[i][f]^2
//   residual : out[c][n] = sigma(Z[n][c]) - y[n]         (the BCE-with-logits gradient factor per checkpoint)
//   cosine / root / scale : the elementwise ends of the three methods, fp64 in, rounded once to fp32
//   topk     : the k extreme entries per row, ties to the lower index
//
// Everything is bit-identical from run to run: no atomics, one fixed summation order.  The moment and squared-distance kernels
// use the Gram kernel's tiling (slab_tiles.h): 64 x 64 output blocks x slabs of the contraction, fp32 partials in a workspace,
// one fold launch that adds the slabs in ascending order in fp64.
//
// moment.  The contraction runs over the rows i, so the A operand of v_mfma_f32_16x16x4_f32 (A[m][k], lane = m + 16 k) is
// X[i0 + lane / 16][f0 + lane % 16] and the B operand the same read at g0: a lane group reads 16 consecutive floats of one row
// and nothing is transposed.  MO_KC = 32 rows x 64 columns of the f block and of the g block go through LDS per step with pitch
// 80 floats (rows k, k + 1, k + 2, k + 3 of one read land in four different quarters of the 64 banks); the weight w[i] is
// multiplied onto the B value as it is read (x * 1.0f where w is absent).  Only blocks with bj >= bi are launched and the fold
// mirrors them.  Rows past the slab's end and columns past F are staged as zeros.
//
// sqdist.  The Gram kernel's staging, then VALU: thread (ti, tj) of 16 x 16 owns rows ti + 16 a and columns tj + 16 b, and every
// entry is one chain acc = fmaf(d, d, acc), d = x - y, over f ascending.  (x - y)^2 == (y - x)^2 and the order is fixed, so with
// X == Y the diagonal is exactly 0 and D is bitwise symmetric.
//
// topk.  A row is cut into chunks of TK_CHUNK = 2048 entries; a workgroup sorts one chunk in LDS (bitonic, 64-bit keys: the
// orderable bits of the value -- inverted for `largest` -- above the index, so ties go to the lower index) and keeps its first k
// keys.  The kept keys of all chunks are a new, shorter row of keys, and the same kernel runs on it until one chunk is left.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "addvisor_hip.h"
#include "common.h"
#include "slab_tiles.h"

namespace advh {

constexpr int MO_KC = 32;              // rows of the contraction staged per step
constexpr int MO_PITCH = GR_BLK + 16;  // LDS row pitch (floats)
constexpr int MO_SLAB_MIN = 512;       // shortest slab (rows)
constexpr int SS_SLAB = 16;            // floats per chain of sumsq
constexpr int TK_CHUNK = 2048;         // entries sorted by one workgroup

struct MomentPlan {
    long slab;   // rows per slab, a multiple of MO_KC
    int nslab, bm;
    long nblk;
};

static MomentPlan moment_plan(long N, int F) {
    MomentPlan p;
    p.bm = (F + GR_BLK - 1) / GR_BLK;
    p.nblk = (long)p.bm * (p.bm + 1) / 2;
    const long maxslabs = GR_TARGET_WG / p.nblk > 1 ? GR_TARGET_WG / p.nblk : 1;
    long slab = (N + maxslabs - 1) / maxslabs;
    slab = (slab + MO_KC - 1) / MO_KC * MO_KC;
    p.slab = slab < MO_SLAB_MIN ? MO_SLAB_MIN : slab;
    p.nslab = (int)((N + p.slab - 1) / p.slab);
    return p;
}

template <bool VEC>
__global__ __launch_bounds__(256) void moment_partial_kernel(const float* __restrict__ X, long ldx, const float* __restrict__ w, long N, int F,
                                                             long slab, int bm, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[MO_KC * MO_PITCH];
    __shared__ __attribute__((aligned(16))) float Bs[MO_KC * MO_PITCH];
    __shared__ float Ws[MO_KC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    int bi, bj;
    block_of((int)blockIdx.x, bm, 1, bi, bj);
    const int f0 = bi * GR_BLK, g0 = bj * GR_BLK;
    const long ibeg = (long)blockIdx.y * slab, iend = ibeg + slab < N ? ibeg + slab : N;
    const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;                   // this wavefront's quarter of the block

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long i0 = ibeg; i0 < iend; i0 += MO_KC) {
        if (i0 != ibeg) __syncthreads();                                 // the previous step's tiles are no longer read
        const int nrow = (int)(iend - i0 < MO_KC ? iend - i0 : MO_KC);
        const float* src = X + i0 * ldx;                                 // rows [0, nrow) of this step
        stage_rows<VEC, MO_KC, GR_BLK, MO_PITCH>(As, src, ldx, 0, nrow, f0, F, tid);
        stage_rows<VEC, MO_KC, GR_BLK, MO_PITCH>(Bs, src, ldx, 0, nrow, g0, F, tid);
        if (tid < MO_KC) Ws[tid] = tid < nrow ? (w ? w[i0 + tid] : 1.f) : 0.f;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MO_KC; kk += 4) {
            const int row = kk + g;
            const float wr = Ws[row];
            float af[2], bf[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = As[row * MO_PITCH + wi + a * 16 + fr];
#pragma unroll
            for (int b = 0; b < 2; ++b) bf[b] = Bs[row * MO_PITCH + wj + b * 16 + fr] * wr;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
    }
    // accumulator layout of the 16 x 16 tile: column = lane % 16, row = 4 (lane / 16) + register
    float* ps = part + (long)blockIdx.y * F * F;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = g0 + wj + b * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = f0 + wi + a * 16 + 4 * g + r;
                if (i < F && j < F) ps[(long)i * F + j] = acc[a][b][r];
            }
        }
}

template <bool VEC>
__global__ __launch_bounds__(256) void sqdist_partial_kernel(const float* __restrict__ X, long ldx, const float* __restrict__ Y, long ldy, int M,
                                                             int N, long F, long slab, int bn, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Xs[GR_BLK * GR_PITCH];
    __shared__ __attribute__((aligned(16))) float Ys[GR_BLK * GR_PITCH];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = ((int)blockIdx.x / bn) * GR_BLK, j0 = ((int)blockIdx.x % bn) * GR_BLK;
    const long kbeg = (long)blockIdx.y * slab, kend = kbeg + slab < F ? kbeg + slab : F;

    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;

    for (long k0 = kbeg; k0 < kend; k0 += GR_KC) {
        if (k0 != kbeg) __syncthreads();
        gram_stage<VEC>(Xs, X, ldx, i0, M, k0, kend, tid);
        gram_stage<VEC>(Ys, Y, ldy, j0, N, k0, kend, tid);
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < GR_KC; kk += 4) {
            float4 xa[4], yb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) xa[a] = *(const float4*)(Xs + (ti + 16 * a) * GR_PITCH + kk);
#pragma unroll
            for (int b = 0; b < 4; ++b) yb[b] = *(const float4*)(Ys + (tj + 16 * b) * GR_PITCH + kk);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float d = xa[a].x - yb[b].x;
                    acc[a][b] = fmaf(d, d, acc[a][b]);
                    d = xa[a].y - yb[b].y;
                    acc[a][b] = fmaf(d, d, acc[a][b]);
                    d = xa[a].z - yb[b].z;
                    acc[a][b] = fmaf(d, d, acc[a][b]);
                    d = xa[a].w - yb[b].w;
                    acc[a][b] = fmaf(d, d, acc[a][b]);
                }
        }
    }
    float* ps = part + (long)blockIdx.y * M * N;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ti + 16 * a, j = j0 + tj + 16 * b;
            if (i < M && j < N) ps[(long)i * N + j] = acc[a][b];
        }
}

// out[i] = sum over the chains of row i, ascending, in fp64; chain q = fmaf(x, x, acc) over floats [16 q, 16 q + 16) from 0.f.
// One workgroup per row, 256 chains per round; thread 0 adds a round's chains in order.
template <bool VEC>
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ X, long ldx, int M, long F, double* __restrict__ out) {
    __shared__ double cs[256];
    const int tid = threadIdx.x;
    const long nchain = (F + SS_SLAB - 1) / SS_SLAB;
    for (int i = (int)blockIdx.x; i < M; i += (int)gridDim.x) {
        const float* row = X + (long)i * ldx;
        double tot = 0.0;
        for (long q0 = 0; q0 < nchain; q0 += 256) {
            const long q = q0 + tid, f = q * SS_SLAB;
            float acc = 0.f;
            if (q < nchain) {
                if (VEC && f + SS_SLAB <= F) {
#pragma unroll
                    for (int v = 0; v < SS_SLAB / 4; ++v) {
                        const float4 t = *(const float4*)(row + f + 4 * v);
                        acc = fmaf(t.x, t.x, acc);
                        acc = fmaf(t.y, t.y, acc);
                        acc = fmaf(t.z, t.z, acc);
                        acc = fmaf(t.w, t.w, acc);
                    }
                } else {
                    const long e = f + SS_SLAB < F ? f + SS_SLAB : F;
                    for (long k = f; k < e; ++k) acc = fmaf(row[k], row[k], acc);
                }
            }
            cs[tid] = (double)acc;
            __syncthreads();
            if (tid == 0) {
                const int n = (int)(nchain - q0 < 256 ? nchain - q0 : 256);
                if (n == 256) {                                              // a full round: the LDS reads are issued ahead of the adds
#pragma unroll 32
                    for (int t = 0; t < 256; ++t) tot += cs[t];
                } else {
                    for (int t = 0; t < n; ++t) tot += cs[t];
                }
            }
            __syncthreads();
        }
        if (tid == 0) out[i] = tot;
    }
}

// sigma in fp64 without overflow: exp of a non-positive number on either side
__device__ __forceinline__ double sigmoid64(double z) {
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}

__global__ __launch_bounds__(256) void residual_kernel(const double* __restrict__ Z, const float* __restrict__ y, long N, int C,
                                                       float* __restrict__ out) {
    const long total = N * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long c = e / N, n = e - c * N;
        const double z = Z[n * C + c], t = (double)y[n];
        out[e] = (float)(t == 1.0 ? -sigmoid64(-z) : sigmoid64(z) - t);     // sigma(z) - 1 == -sigma(-z): no cancellation near 1
    }
}

// mode 0: G / (sqrt(a[m]) sqrt(b[n])), 0 where a norm is zero; mode 1: sqrt(G) (a, b unused)
__global__ __launch_bounds__(256) void cosine_kernel(const double* __restrict__ G, const double* __restrict__ a, const double* __restrict__ b,
                                                     int M, long N, int mode, float* __restrict__ out, long ldo) {
    const long total = (long)M * N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long m = e / N, n = e - m * N;
        double v;
        if (mode) {
            v = sqrt(G[e]);
        } else {
            const double am = a[m], bn = b[n];
            v = (am == 0.0 || bn == 0.0) ? 0.0 : G[e] / (sqrt(am) * sqrt(bn));
        }
        out[m * ldo + n] = (float)v;
    }
}

// out[m][n] = G[m][n] * sum_c (lr[c] * rt[c][m]) * rn[c][n]: c ascending, every product and sum rounded on its own (no fma)
__global__ __launch_bounds__(256) void scale_kernel(const double* __restrict__ G, const float* __restrict__ rt, const float* __restrict__ rn,
                                                    const double* __restrict__ lr, int C, int M, long N, float* __restrict__ out, long ldo) {
#pragma clang fp contract(off)
    const long total = (long)M * N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long m = e / N, n = e - m * N;
        double s = 0.0;
        for (int c = 0; c < C; ++c) s = s + (lr[c] * (double)rt[(long)c * M + m]) * (double)rn[(long)c * N + n];
        out[m * ldo + n] = (float)(G[e] * s);
    }
}

// out[n] = ss[n] * sum_c (lr[c] * rn[c][n]) * rn[c][n]: the diagonal of the scale kernel's product, same rounding
__global__ __launch_bounds__(256) void self_scale_kernel(const double* __restrict__ ss, const float* __restrict__ rn, const double* __restrict__ lr,
                                                         int C, long N, float* __restrict__ out) {
#pragma clang fp contract(off)
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
            const double r = (double)rn[(long)c * N + n];
            s = s + (lr[c] * r) * r;
        }
        out[n] = (float)(ss[n] * s);
    }
}

// ascending unsigned order == ascending float order; -0.0 counts as +0.0 (numpy's comparison)
__device__ __forceinline__ uint32_t orderable(float v) {
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One chunk of one row: keys from S (keys_in == nullptr) or from the kept keys of the previous pass; sorted ascending; the first
// k go to keys_out [row][chunk][k], or -- the last pass, keys_out == nullptr -- to idx / val.
__global__ __launch_bounds__(256) void topk_pass_kernel(const float* __restrict__ S, long lds, const uint64_t* __restrict__ keys_in, long n_in,
                                                        long in_stride, int k, int largest, uint64_t* __restrict__ keys_out,
                                                        int* __restrict__ idx, float* __restrict__ val) {
    __shared__ uint64_t ks[TK_CHUNK];
    const int tid = threadIdx.x;
    const long m = blockIdx.y, c0 = (long)blockIdx.x * TK_CHUNK;
#pragma unroll
    for (int q = 0; q < TK_CHUNK / 256; ++q) {
        const int t = tid + 256 * q;
        const long e = c0 + t;
        uint64_t key = ~0ull;                                            // padding: after every entry
        if (e < n_in) {
            if (keys_in) {
                key = keys_in[m * in_stride + e];
            } else {
                const uint32_t o = orderable(S[m * lds + e]);
                key = ((uint64_t)(largest ? ~o : o) << 32) | (uint64_t)e;
            }
        }
        ks[t] = key;
    }
    __syncthreads();
    for (int size = 2; size <= TK_CHUNK; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int q = 0; q < TK_CHUNK / 512; ++q) {
                const int p = tid + 256 * q;
                const int lo = 2 * j * (p / j) + (p % j), hi = lo + j;
                const uint64_t a = ks[lo], b = ks[hi];
                const bool up = (lo & size) == 0;
                if ((a > b) == up) { ks[lo] = b; ks[hi] = a; }
            }
            __syncthreads();
        }
    for (int t = tid; t < k; t += 256) {
        const uint64_t key = ks[t];
        if (keys_out) {
            keys_out[(m * gridDim.x + blockIdx.x) * k + t] = key;
        } else {
            const uint32_t e = (uint32_t)key;
            idx[m * k + t] = (int)e;
            val[m * k + t] = S[m * lds + e];
        }
    }
}

}  // namespace advh

using namespace advh;

constexpr long GRID_CAP = 16384;   // blocks of the grid-stride kernels

static bool moment_args_ok(int64_t N, int F) { return N > 0 && N <= (1LL << 24) && F > 0 && F <= 4096; }

extern "C" int64_t advh_influence_moment_workspace(int64_t N, int F) {
    if (!moment_args_ok(N, F)) return ADVH_EINVAL;
    return (int64_t)moment_plan((long)N, F).nslab * F * F * (int64_t)sizeof(float);
}

extern "C" int advh_influence_moment(const float* X, int64_t ldx, const float* w, int64_t N, int F, float* workspace, double* Hm,
                                     advh_stream_t stream) {
    if (!X || !workspace || !Hm || !moment_args_ok(N, F) || ldx < F) return ADVH_EINVAL;
    if (((uintptr_t)X & 3) || ((uintptr_t)w & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)Hm & 7)) return ADVH_EINVAL;
    const MomentPlan p = moment_plan((long)N, F);
    const bool vec = aligned16(X) && ldx % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    launch_vec(vec, moment_partial_kernel<true>, moment_partial_kernel<false>, dim3((unsigned)p.nblk, (unsigned)p.nslab), s, X, ldx, w, N, F,
               p.slab, p.bm, workspace);
    if (ADVH_LAUNCH_CHECK() != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL(gram_fold_kernel<double>, dim3(grid_for((long)F * F, GRID_CAP)), dim3(256), 0, s, workspace, F, F, p.nslab, 1, Hm);
    return ADVH_LAUNCH_CHECK();
}

static bool sqdist_args_ok(int M, int N, int64_t F) { return M > 0 && N > 0 && F > 0 && M <= (1 << 20) && N <= (1 << 20) && F <= (1LL << 40); }

extern "C" int64_t advh_influence_sqdist_workspace(int M, int N, int64_t F) {
    if (!sqdist_args_ok(M, N, F)) return ADVH_EINVAL;
    return (int64_t)gram_plan(M, N, (long)F, 0).nslab * M * N * (int64_t)sizeof(float);
}

extern "C" int advh_influence_sqdist(const float* X, int64_t ldx, const float* Y, int64_t ldy, int M, int N, int64_t F, float* workspace,
                                     double* D, advh_stream_t stream) {
    if (!X || !Y || !workspace || !D || !sqdist_args_ok(M, N, F) || ldx < F || ldy < F) return ADVH_EINVAL;
    if (((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)D & 7)) return ADVH_EINVAL;
    const GramPlan p = gram_plan(M, N, (long)F, 0);
    if (p.nblk > 0x7fffffffL || p.nslab > 65535) return ADVH_EUNSUPPORTED;
    const bool vec = aligned16(X) && aligned16(Y) && ldx % 4 == 0 && ldy % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    launch_vec(vec, sqdist_partial_kernel<true>, sqdist_partial_kernel<false>, dim3((unsigned)p.nblk, (unsigned)p.nslab), s, X, ldx, Y, ldy, M, N,
               F, p.slab, p.bn, workspace);
    if (ADVH_LAUNCH_CHECK() != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL(gram_fold_kernel<double>, dim3(grid_for((long)M * N, GRID_CAP)), dim3(256), 0, s, workspace, M, N, p.nslab, 0, D);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_influence_sumsq(const float* X, int64_t ldx, int M, int64_t F, double* out, advh_stream_t stream) {
    if (!X || !out || M <= 0 || M > (1 << 24) || F <= 0 || F > (1LL << 40) || ldx < F) return ADVH_EINVAL;
    if (((uintptr_t)X & 3) || ((uintptr_t)out & 7)) return ADVH_EINVAL;
    const bool vec = aligned16(X) && ldx % 4 == 0;
    launch_vec(vec, sumsq_kernel<true>, sumsq_kernel<false>, dim3((unsigned)(M < GRID_CAP ? M : GRID_CAP)), (hipStream_t)stream, X, ldx, M, F, out);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_influence_residual(const double* Z, const float* y, int64_t N, int C, float* out, advh_stream_t stream) {
    if (!Z || !y || !out || N <= 0 || N > (1LL << 24) || C <= 0 || C > 65536) return ADVH_EINVAL;
    if (((uintptr_t)Z & 7) || ((uintptr_t)y & 3) || ((uintptr_t)out & 3)) return ADVH_EINVAL;
    hipLaunchKernelGGL(residual_kernel, dim3(grid_for((long)N * C, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, Z, y, (long)N, C, out);
    return ADVH_LAUNCH_CHECK();
}

static bool matrix_args_ok(int M, int64_t N, int64_t ldo) { return M > 0 && M <= (1 << 20) && N > 0 && N <= (1LL << 24) && ldo >= N; }

extern "C" int advh_influence_cosine(const double* G, const double* a, const double* b, int M, int64_t N, float* out, int64_t ldo,
                                     advh_stream_t stream) {
    if (!G || !a || !b || !out || !matrix_args_ok(M, N, ldo)) return ADVH_EINVAL;
    if (((uintptr_t)G & 7) || ((uintptr_t)a & 7) || ((uintptr_t)b & 7) || ((uintptr_t)out & 3)) return ADVH_EINVAL;
    hipLaunchKernelGGL(cosine_kernel, dim3(grid_for((long)M * N, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, G, a, b, M, (long)N, 0, out,
                       (long)ldo);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_influence_root(const double* D, int M, int64_t N, float* out, int64_t ldo, advh_stream_t stream) {
    if (!D || !out || !matrix_args_ok(M, N, ldo)) return ADVH_EINVAL;
    if (((uintptr_t)D & 7) || ((uintptr_t)out & 3)) return ADVH_EINVAL;
    hipLaunchKernelGGL(cosine_kernel, dim3(grid_for((long)M * N, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, D, (const double*)nullptr,
                       (const double*)nullptr, M, (long)N, 1, out, (long)ldo);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_influence_scale(const double* G, const float* rt, const float* rn, const double* lr, int C, int M, int64_t N, float* out,
                                    int64_t ldo, advh_stream_t stream) {
    if (!G || !rt || !rn || !lr || !out || C <= 0 || C > 65536 || !matrix_args_ok(M, N, ldo)) return ADVH_EINVAL;
    if (((uintptr_t)G & 7) || ((uintptr_t)lr & 7) || ((uintptr_t)rt & 3) || ((uintptr_t)rn & 3) || ((uintptr_t)out & 3)) return ADVH_EINVAL;
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for((long)M * N, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, G, rt, rn, lr, C, M, (long)N, out,
                       (long)ldo);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_influence_self_scale(const double* ss, const float* rn, const double* lr, int C, int64_t N, float* out,
                                         advh_stream_t stream) {
    if (!ss || !rn || !lr || !out || C <= 0 || C > 65536 || N <= 0 || N > (1LL << 24)) return ADVH_EINVAL;
    if (((uintptr_t)ss & 7) || ((uintptr_t)lr & 7) || ((uintptr_t)rn & 3) || ((uintptr_t)out & 3)) return ADVH_EINVAL;
    hipLaunchKernelGGL(self_scale_kernel, dim3(grid_for((long)N, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, ss, rn, lr, C, (long)N, out);
    return ADVH_LAUNCH_CHECK();
}

static bool topk_args_ok(int M, int64_t N, int k) { return M > 0 && M <= 65535 && N > 0 && N <= (1LL << 24) && k >= 1 && k <= 256 && k <= N; }

static long chunks_of(long n) { return (n + TK_CHUNK - 1) / TK_CHUNK; }

extern "C" int64_t advh_influence_topk_workspace(int M, int64_t N, int k) {
    if (!topk_args_ok(M, N, k)) return ADVH_EINVAL;
    const long c1 = chunks_of((long)N), c2 = chunks_of(c1 * k);
    const long keys = (c1 > 1 ? c1 : 0) + (c1 > 1 && c2 > 1 ? c2 : 0);
    const int64_t bytes = 8LL * M * k * keys;
    return bytes < 16 ? 16 : bytes;
}

extern "C" int advh_influence_topk(const float* S, int64_t lds, int M, int64_t N, int k, int largest, void* workspace, int* idx, float* val,
                                   advh_stream_t stream) {
    if (!S || !workspace || !idx || !val || !topk_args_ok(M, N, k) || lds < N || (largest != 0 && largest != 1)) return ADVH_EINVAL;
    if (((uintptr_t)S & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)idx & 3) || ((uintptr_t)val & 3)) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    uint64_t* buf[2] = {(uint64_t*)workspace, (uint64_t*)workspace + (long)M * k * chunks_of((long)N)};
    const uint64_t* in = nullptr;
    long n_in = (long)N;
    for (int pass = 0;; ++pass) {
        const long nc = chunks_of(n_in);
        uint64_t* outk = nc > 1 ? buf[pass & 1] : nullptr;               // one chunk left: the last pass
        hipLaunchKernelGGL(topk_pass_kernel, dim3((unsigned)nc, (unsigned)M), dim3(256), 0, s, S, (long)lds, in, n_in, n_in, k, largest, outk, idx,
                           val);
        if (ADVH_LAUNCH_CHECK() != ADVH_OK) return ADVH_ELAUNCH;
        if (!outk) return ADVH_OK;
        in = outk;
        n_in = nc * k;
    }
}
