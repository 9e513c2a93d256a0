// Permuted batches of Captum's FeaturePermutation, the per-row similarity weights of Captum's Lime, and Lime's Lasso solve on the
// host: include/addvisor_hip.h, advh_permutation_points / advh_row_similarity / advh_lasso_cd.
//
// The two kernels are memory-bound and tiny next to the classifier forwards they serve (one forward row is on the order of a
// GFLOP), so they stay simple: float4 access when every row pointer is 16-byte aligned (base pointers aligned and n % 4 == 0),
// a scalar path otherwise.  The permuted rows are a rule of the row-building skeleton, csrc/attribution_rows.h.
//
// Determinism contract of advh_row_similarity: one workgroup per row; thread t adds the quads t, t + 256, ... in order, the four
// elements of a quad in order (the scalar path visits the same elements in the same order, so both paths give the same bits), in
// fp64; then a wave64 __shfl_xor tree and the four waves as (w0 + w1) + (w2 + w3).  A row's weight depends only on the row and
// its clip, never on the chunk it came in.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_rows.h"
#include "common.h"

namespace advh {

enum { SIM_COSINE = 0, SIM_EUCLIDEAN = 1 };

// The permuted rows (csrc/attribution_rows.h): row g = k * B + b is x[b] with x[perm[k][b]][t] where index[t] == k; rows
// g >= K * B are padding.  A perm entry outside [0, B) gives NaN on the samples of feature k (no read outside x).
struct PermutationRule {
    advh_permutation_desc c;
    __host__ __device__ long n() const { return c.n; }
    struct Row {
        long k;     // < 0: a padding row
        bool bad;   // the perm entry is outside [0, B)
        const float *xr, *pr;
    };
    __device__ __forceinline__ Row row(long g) const {
        const long b = g % c.B, k = g < (long)c.K * c.B ? g / c.B : -1L;
        const int src = k >= 0 ? c.perm[g] : (int)b;                             // the table is [K][B]: entry k * B + b = g
        const bool bad = src < 0 || src >= c.B;
        return {k, bad, c.x + b * c.n, c.x + (bad ? b : (long)src) * c.n};
    }
    // the partner row is read only when one of the four samples belongs to feature k
    __device__ __forceinline__ float4 quad(const Row& w, long t) const {
        float4 v = *(const float4*)(w.xr + t);
        if (w.k >= 0) {
            const int4 id = *(const int4*)(c.index + t);
            const bool m0 = id.x == w.k, m1 = id.y == w.k, m2 = id.z == w.k, m3 = id.w == w.k;
            if (m0 || m1 || m2 || m3) {
                const float4 pv = w.bad ? make_float4(NAN, NAN, NAN, NAN) : *(const float4*)(w.pr + t);
                v = make_float4(m0 ? pv.x : v.x, m1 ? pv.y : v.y, m2 ? pv.z : v.z, m3 ? pv.w : v.w);
            }
        }
        return v;
    }
    __device__ __forceinline__ float one(const Row& w, long t) const {
        const bool m = w.k >= 0 && c.index[t] == w.k;
        return m ? (w.bad ? NAN : w.pr[t]) : w.xr[t];
    }
};

// Fixed-shape workgroup sum of N fp64 values per thread (256 threads): wave64 xor tree, then (w0 + w1) + (w2 + w3).  Valid in
// thread 0.
template <int N>
__device__ __forceinline__ void block_sum(double (&s)[N]) {
    __shared__ double red[4][N];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int j = 0; j < N; ++j) s[j] += __shfl_xor(s[j], o, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < N; ++j) red[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}

// Accumulates one element pair (clip value a, row value v) into the mode's sums.
template <int MODE>
__device__ __forceinline__ void sim_acc(double (&s)[MODE == SIM_COSINE ? 3 : 1], float a, float v) {
    const double xa = a, xv = v;
    if (MODE == SIM_COSINE) {
        s[0] += xa * xv;
        s[1] += xa * xa;
        s[2] += xv * xv;
    } else {
        const double d = xa - xv;
        s[0] += d * d;
    }
}

// sim[row0 + r] = exp(-d^2 / (2 w^2)) of chunk row r against its clip x[(row0 + r) % B]; one workgroup per row.
//   cosine:    d = 1 - <x, v> / (max(||x||, 1e-8) * max(||v||, 1e-8))   (torch.nn.CosineSimilarity(dim=0))
//   euclidean: d^2 = ||x - v||^2
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void row_similarity_kernel(const float* __restrict__ rows, const float* __restrict__ x, long row0, int B,
                                                             long n, double inv_2w2, float* __restrict__ sim) {
    constexpr int N = MODE == SIM_COSINE ? 3 : 1;
    const long r = blockIdx.x, g = row0 + r;
    const float* vr = rows + r * n;
    const float* xr = x + (g % B) * n;
    const long nq = (n + 3) / 4;
    double s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.0;
    for (long q = threadIdx.x; q < nq; q += 256) {
        if (VEC) {
            const float4 a = *(const float4*)(xr + q * 4), v = *(const float4*)(vr + q * 4);
            sim_acc<MODE>(s, a.x, v.x);
            sim_acc<MODE>(s, a.y, v.y);
            sim_acc<MODE>(s, a.z, v.z);
            sim_acc<MODE>(s, a.w, v.w);
        } else {
            for (int k = 0; k < 4; ++k) {
                const long j = q * 4 + k;
                if (j >= n) break;
                sim_acc<MODE>(s, xr[j], vr[j]);
            }
        }
    }
    block_sum<N>(s);
    if (threadIdx.x == 0) {
        double d2;
        if (MODE == SIM_COSINE) {
            const double d = 1.0 - s[0] / (fmax(sqrt(s[1]), 1e-8) * fmax(sqrt(s[2]), 1e-8));
            d2 = d * d;
        } else {
            d2 = s[0];
        }
        sim[g] = (float)exp(-d2 * inv_2w2);
    }
}

}  // namespace advh

using namespace advh;

extern "C" int advh_permutation_points(const advh_permutation_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    if (!d || !d->x || !d->index || !d->perm || !out || d->n <= 0 || d->B < 2 || d->K <= 0 || row0 < 0 || rows < 0) return ADVH_EINVAL;
    const bool vec = d->n % 4 == 0 && aligned16(d->x) && aligned16(d->index) && aligned16(out);
    return build_rows(PermutationRule{*d}, vec, (long)row0, rows, out, (hipStream_t)stream);
}

extern "C" int advh_row_similarity(const float* rows_ptr, const float* x, int64_t row0, int rows, int B, int64_t n, int mode,
                                   float kernel_width, float* sim, advh_stream_t stream) {
    if (!rows_ptr || !x || !sim || row0 < 0 || rows < 0 || B <= 0 || n <= 0) return ADVH_EINVAL;
    if ((mode != SIM_COSINE && mode != SIM_EUCLIDEAN) || !(kernel_width > 0.f) || isinf(kernel_width)) return ADVH_EINVAL;
    if (rows == 0) return ADVH_OK;
    const double w = kernel_width, inv_2w2 = 1.0 / (2.0 * w * w);
    const bool vec = n % 4 == 0 && aligned16(rows_ptr) && aligned16(x);
    const hipStream_t s = (hipStream_t)stream;
    if (mode == SIM_COSINE)
        launch_vec(vec, row_similarity_kernel<SIM_COSINE, true>, row_similarity_kernel<SIM_COSINE, false>, dim3(rows), s, rows_ptr, x, row0, B, n,
                   inv_2w2, sim);
    else
        launch_vec(vec, row_similarity_kernel<SIM_EUCLIDEAN, true>, row_similarity_kernel<SIM_EUCLIDEAN, false>, dim3(rows), s, rows_ptr, x, row0,
                   B, n, inv_2w2, sim);
    return ADVH_LAUNCH_CHECK();
}

// Host: cyclic coordinate descent of 1/2 ||y - X c||^2 + alpha ||c||_1 (sklearn's enet_coordinate_descent with l2 = 0), X given
// column by column.  The duality gap is evaluated whenever the largest coordinate step of a sweep is below tol relative to the
// largest coefficient (and after the last sweep), on a residual recomputed from scratch; the solve stops when it is below
// tol * ||y||^2.
extern "C" int advh_lasso_cd(const double* X, const double* y, int S, int K, double alpha, double tol, int max_iter, double* coef,
                             double* gap_out, int* iters_out) {
    if (!X || !y || !coef || !gap_out || !iters_out || S <= 0 || K <= 0 || max_iter < 1) return ADVH_EINVAL;
    if (!(alpha >= 0.0) || isinf(alpha) || !(tol >= 0.0) || isinf(tol)) return ADVH_EINVAL;
    double* norm2 = new double[K];
    double* R = new double[S];
    double yy = 0.0;
    for (int s = 0; s < S; ++s) yy += y[s] * y[s];
    for (int k = 0; k < K; ++k) {
        const double* xk = X + (long)k * S;
        double a = 0.0;
        for (int s = 0; s < S; ++s) a += xk[s] * xk[s];
        norm2[k] = a;
    }
    auto residual = [&]() {
        for (int s = 0; s < S; ++s) R[s] = y[s];
        for (int k = 0; k < K; ++k) {
            if (coef[k] == 0.0) continue;
            const double* xk = X + (long)k * S;
            for (int s = 0; s < S; ++s) R[s] -= coef[k] * xk[s];
        }
    };
    auto gap = [&]() {
        residual();
        double dual = 0.0, r2 = 0.0, ry = 0.0, l1 = 0.0;
        for (int k = 0; k < K; ++k) {
            const double* xk = X + (long)k * S;
            double a = 0.0;
            for (int s = 0; s < S; ++s) a += xk[s] * R[s];
            dual = fmax(dual, fabs(a));
            l1 += fabs(coef[k]);
        }
        for (int s = 0; s < S; ++s) {
            r2 += R[s] * R[s];
            ry += R[s] * y[s];
        }
        double cst = 1.0, g;
        if (dual > alpha) {
            cst = alpha / dual;
            g = 0.5 * (r2 + r2 * cst * cst);
        } else {
            g = r2;
        }
        return g + alpha * l1 - cst * ry;
    };
    residual();
    const double tol_abs = tol * yy;
    double g = INFINITY;
    int it = 0;
    while (it < max_iter) {
        ++it;
        double w_max = 0.0, dw_max = 0.0;
        for (int k = 0; k < K; ++k) {
            if (norm2[k] == 0.0) continue;
            const double* xk = X + (long)k * S;
            const double old = coef[k];
            double a = 0.0;
            for (int s = 0; s < S; ++s) a += xk[s] * R[s];
            a += norm2[k] * old;                                           // X_k . (R + X_k c_k)
            const double c = a > alpha ? (a - alpha) / norm2[k] : a < -alpha ? (a + alpha) / norm2[k] : 0.0;
            if (c != old) {
                const double dc = c - old;
                for (int s = 0; s < S; ++s) R[s] -= dc * xk[s];
                coef[k] = c;
            }
            dw_max = fmax(dw_max, fabs(c - old));
            w_max = fmax(w_max, fabs(c));
        }
        if (w_max == 0.0 || dw_max / w_max <= tol || it == max_iter) {
            g = gap();
            if (g <= tol_abs) break;
        }
    }
    *gap_out = g;
    *iters_out = it;
    delete[] norm2;
    delete[] R;
    return ADVH_OK;
}
