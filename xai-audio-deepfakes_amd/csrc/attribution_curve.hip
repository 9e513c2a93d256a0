// Perturbation curves of any attribution map (deletion / insertion AUC, AOPC in MoRF / LeRF order): include/addvisor_hip.h,
// advh_feature_scores / advh_feature_rank / advh_curve_points / advh_curve_fold.
//
// These kernels are tiny next to the classifier forwards they serve, so they stay simple and deterministic: no atomics, every
// sum and count in a fixed order, bit-identical from run to run.  The curve rows are a rule of the row-building skeleton,
// csrc/attribution_rows.h.
//
// Order contract of the scores: score[b][k] adds the samples of feature k sequentially in increasing t from 0.f, so that a
// sequential fp32 replay on the host gives the same bits.  One thread owns one feature; the workgroup stages SC_TILE samples
// (feature index, value) in LDS, and every thread walks the tile in order adding its own samples -- all lanes read the same LDS
// words, a broadcast.  A tile none of whose samples belongs to the workgroup's 256 features is skipped (__syncthreads_or), which
// makes contiguous segments cost O(n + K * SC_TILE) instead of O(K * n).
//
// Rank: one path for every K.  rank[b][k] = #{j : key_j < key_k} over packed 64-bit keys (ordered score bits, or their
// complement for the descending order, in the high word; the feature number in the low word), so the tie rule "equal scores:
// lower feature first" is the key order itself and the keys of a clip are distinct: the ranks are a permutation of [0, K) by
// construction.  Keys are staged RK_TILE at a time in LDS (16 KB) and read as broadcasts; a thread carries RK_ITEMS features
// in registers so that one LDS read feeds RK_ITEMS comparisons.  K * K comparisons per clip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "addvisor_hip.h"
#include "attribution_rows.h"
#include "common.h"

namespace advh {

enum { CURVE_DELETION = 0, CURVE_INSERTION = 1 };
constexpr int SC_TILE = 1024;                 // samples staged per step of the score kernel
constexpr int RK_ITEMS = 4, RK_TILE = 2048;   // features per thread / keys staged per step of the rank kernel

// score[b][k] for k = blockIdx.x * 256 + threadIdx.x of clip blockIdx.y
__global__ __launch_bounds__(256) void feature_scores_kernel(const float* __restrict__ attr, const int32_t* __restrict__ index,
                                                             int index_rows, long n, int K, int use_abs, int mean,
                                                             float* __restrict__ score) {
    __shared__ __attribute__((aligned(16))) int sidx[SC_TILE];
    __shared__ __attribute__((aligned(16))) float sval[SC_TILE];
    const int tid = threadIdx.x, k0 = blockIdx.x * 256, k = k0 + tid;
    const long b = blockIdx.y;
    const float* ar = attr + b * n;
    const int32_t* ir = index + (index_rows == 1 ? 0L : b * n);
    float acc = 0.f;
    int cnt = 0;
    for (long t0 = 0; t0 < n; t0 += SC_TILE) {
        const int len = (int)min((long)SC_TILE, n - t0);
        int hit = 0;
        for (int i = tid; i < SC_TILE; i += 256) {                       // past the end: index -1, nobody's sample
            const int f = i < len ? ir[t0 + i] : -1;
            const float v = i < len ? ar[t0 + i] : 0.f;
            sidx[i] = f;
            sval[i] = use_abs ? fabsf(v) : v;
            hit |= (f >= k0 && f < k0 + 256) ? 1 : 0;
        }
        if (__syncthreads_or(hit)) {
            // Branch-free, so that the LDS reads run ahead of the dependent adds: acc starts at +0 and an fp32 sum never
            // becomes -0 from there (x + (-x) = +0), so adding +0.f for another feature's sample changes no bit of acc.
#pragma unroll 4
            for (int i = 0; i < SC_TILE; i += 4) {
                const int4 f = *(const int4*)(sidx + i);
                const float4 v = *(const float4*)(sval + i);
                acc += f.x == k ? v.x : 0.f;
                acc += f.y == k ? v.y : 0.f;
                acc += f.z == k ? v.z : 0.f;
                acc += f.w == k ? v.w : 0.f;
                cnt += (f.x == k) + (f.y == k) + (f.z == k) + (f.w == k);
            }
        }
        __syncthreads();
    }
    if (k < K) score[b * K + k] = cnt == 0 ? -INFINITY : mean ? __fdiv_rn(acc, (float)cnt) : acc;
}

// the identity index (K == n, every sample its own feature): a sum of one term, a mean over one sample
__global__ __launch_bounds__(256) void feature_scores_identity_kernel(const float* __restrict__ attr, long total, int use_abs,
                                                                      float* __restrict__ score) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float v = 0.f + (use_abs ? fabsf(attr[i]) : attr[i]);      // 0.f + v: the sum's first step (-0 becomes +0)
        score[i] = v;
    }
}

// The order key of feature j: ascending in the score (descending: in its negation), then in j.  -0 counts as +0.
__device__ __forceinline__ uint64_t rank_key(float s, int j, int descending) {
    unsigned u = __float_as_uint(s);
    if ((u << 1) == 0u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (descending) u = ~u;
    return ((uint64_t)u << 32) | (unsigned)j;
}

// rank[b][k] for the RK_ITEMS features k = blockIdx.x * 256 * RK_ITEMS + i * 256 + threadIdx.x of clip blockIdx.y
__global__ __launch_bounds__(256) void feature_rank_kernel(const float* __restrict__ score, int K, int descending,
                                                           int32_t* __restrict__ rank) {
    __shared__ uint64_t skey[RK_TILE];
    const int tid = threadIdx.x, k0 = blockIdx.x * 256 * RK_ITEMS;
    const float* sr = score + (long)blockIdx.y * K;
    uint64_t mine[RK_ITEMS];
    int before[RK_ITEMS];
#pragma unroll
    for (int q = 0; q < RK_ITEMS; ++q) {
        const int k = k0 + q * 256 + tid;
        mine[q] = k < K ? rank_key(sr[k], k, descending) : 0ull;         // key 0: nothing comes before it, and it is not stored
        before[q] = 0;
    }
    for (int j0 = 0; j0 < K; j0 += RK_TILE) {
        const int len = min(RK_TILE, K - j0);
        for (int i = tid; i < len; i += 256) skey[i] = rank_key(sr[j0 + i], j0 + i, descending);
        __syncthreads();
        for (int i = 0; i < len; ++i) {
            const uint64_t kj = skey[i];
#pragma unroll
            for (int q = 0; q < RK_ITEMS; ++q) before[q] += kj < mine[q] ? 1 : 0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < RK_ITEMS; ++q) {
        const int k = k0 + q * 256 + tid;
        if (k < K) rank[(long)blockIdx.y * K + k] = before[q];
    }
}

// The curve rows (csrc/attribution_rows.h): row g is step j = g / B of clip b = g % B; rows g >= S1 * B are padding.
struct CurveRule {
    advh_curve_desc c;
    __host__ __device__ long n() const { return c.n; }
    struct Row {
        bool pad;
        int count;   // features switched at this step
        const float *xr, *br;
        const int32_t *ir, *rr;   // ir == nullptr: the identity index
    };
    __device__ __forceinline__ Row row(long g) const {
        const long j = g / c.B, b = g - j * c.B;
        const bool pad = g >= (long)c.S1 * c.B;
        return {pad, pad ? 0 : c.counts[j], c.x + b * c.n, c.base + (c.base_rows == 1 ? 0L : b * c.n),
                c.index ? c.index + (c.index_rows == 1 ? 0L : b * c.n) : nullptr, c.rank + b * c.K};
    }
    // The value of a sample of feature f: switched when rank[b][f] < count.
    __device__ __forceinline__ float pick(const Row& w, int f, float xv, float bv) const {
        if (f < 0 || f >= c.K) return NAN;
        const bool switched = w.rr[f] < w.count;
        return (switched == (c.mode == CURVE_DELETION)) ? bv : xv;
    }
    __device__ __forceinline__ float4 quad(const Row& w, long t) const {
        const float4 xv = *(const float4*)(w.xr + t);
        if (w.pad) return xv;
        const float4 bv = *(const float4*)(w.br + t);
        const int4 id = w.ir ? *(const int4*)(w.ir + t) : make_int4((int)t, (int)t + 1, (int)t + 2, (int)t + 3);
        return make_float4(pick(w, id.x, xv.x, bv.x), pick(w, id.y, xv.y, bv.y), pick(w, id.z, xv.z, bv.z), pick(w, id.w, xv.w, bv.w));
    }
    __device__ __forceinline__ float one(const Row& w, long t) const {
        return w.pad ? w.xr[t] : pick(w, w.ir ? w.ir[t] : (int)t, w.xr[t], w.br[t]);
    }
};

// One thread per clip, steps in increasing j: curve[b][j] = y_j, auc and aopc accumulated in fp64 and rounded once.  Counts that
// are not strictly increasing inside [0, K] (they live on the device: the host cannot see them) give NaN in auc and aopc.
__global__ __launch_bounds__(64) void curve_fold_kernel(const float* __restrict__ fk, const int32_t* __restrict__ counts, int B, int S1,
                                                        int K, int prob, int ref_last, float* __restrict__ curve,
                                                        float* __restrict__ auc, float* __restrict__ aopc) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int ref = ref_last ? S1 - 1 : 0;
    double area = 0.0, drop = 0.0, y_prev = 0.0, y_ref = 0.0;
    bool ok = true;
    // y_ref first: the sum runs over j in increasing order and needs it from the start
    {
        const float z = fk[(long)ref * B + b];
        y_ref = prob ? __fdiv_rn(1.f, 1.f + expf(-z)) : z;
    }
    for (int j = 0; j < S1; ++j) {
        const float z = fk[(long)j * B + b];
        const float yf = prob ? __fdiv_rn(1.f, 1.f + expf(-z)) : z;
        curve[(long)b * S1 + j] = yf;
        const double y = yf;
        const int cj = counts[j];
        ok = ok && cj >= 0 && cj <= K;
        if (j > 0) {
            const int cp = counts[j - 1];
            ok = ok && cp < cj;
            area += ((double)cj / K - (double)cp / K) * (y_prev + y) * 0.5;
        }
        if (j != ref) drop += y_ref - y;
        y_prev = y;
    }
    const double span = (double)counts[S1 - 1] / K - (double)counts[0] / K;
    auc[b] = ok ? (float)(area / span) : NAN;
    aopc[b] = ok ? (float)(drop / (double)(S1 - 1)) : NAN;
}

}  // namespace advh

using namespace advh;

extern "C" int advh_feature_scores(const float* attr, const int32_t* index, int index_rows, int B, int64_t n, int K, int use_abs, int mean,
                                   float* score, advh_stream_t stream) {
    if (!attr || !score || B <= 0 || n <= 0 || K <= 0 || K > n || B > 65535) return ADVH_EINVAL;
    if (index ? (index_rows != 1 && index_rows != B) : K != n) return ADVH_EINVAL;
    if (!index)
        hipLaunchKernelGGL(feature_scores_identity_kernel, dim3(grid_for((long)B * n)), dim3(256), 0, (hipStream_t)stream, attr, (long)B * n,
                           use_abs, score);
    else
        hipLaunchKernelGGL(feature_scores_kernel, dim3((K + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, attr, index, index_rows,
                           (long)n, K, use_abs, mean, score);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_feature_rank(const float* score, int B, int K, int descending, int32_t* rank, advh_stream_t stream) {
    if (!score || !rank || B <= 0 || K <= 0 || B > 65535) return ADVH_EINVAL;
    const int per = 256 * RK_ITEMS;
    hipLaunchKernelGGL(feature_rank_kernel, dim3((K + per - 1) / per, B), dim3(256), 0, (hipStream_t)stream, score, K, descending ? 1 : 0,
                       rank);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_curve_points(const advh_curve_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    if (!d || !d->x || !d->base || !d->rank || !d->counts || !out || d->B <= 0 || d->n <= 0 || d->K <= 0 || d->K > d->n) return ADVH_EINVAL;
    if (d->base_rows != 1 && d->base_rows != d->B) return ADVH_EINVAL;
    if (d->index ? (d->index_rows != 1 && d->index_rows != d->B) : d->K != d->n) return ADVH_EINVAL;
    if (d->mode != CURVE_DELETION && d->mode != CURVE_INSERTION) return ADVH_EINVAL;
    if (d->S1 < 1 || d->S1 > d->K + 1 || row0 < 0 || rows < 0) return ADVH_EINVAL;     // S1 strictly increasing counts fit [0, K]
    const bool vec = d->n % 4 == 0 && aligned16(d->x) && aligned16(d->base) && aligned16(out) && aligned16(d->index);
    return build_rows(CurveRule{*d}, vec, (long)row0, rows, out, (hipStream_t)stream);
}

extern "C" int advh_curve_fold(const float* fk, const int32_t* counts, int B, int S1, int K, int prob, int ref_last, float* curve, float* auc,
                               float* aopc, advh_stream_t stream) {
    if (!fk || !counts || !curve || !auc || !aopc || B <= 0 || K <= 0 || S1 < 2 || S1 > K + 1) return ADVH_EINVAL;
    hipLaunchKernelGGL(curve_fold_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, fk, counts, B, S1, K, prob ? 1 : 0,
                       ref_last ? 1 : 0, curve, auc, aopc);
    return ADVH_LAUNCH_CHECK();
}
