// Time-frequency attributions over the STFT mask (include/addvisor_hip.h): Captum's Occlusion for a (Fm, Tm) input --
// advh_occlusion2d_points / advh_occlusion2d_accumulate -- and the band x segment pooling of an attribution map, advh_tf_pool.
//
// The occlusion kernels are the 2-D form of csrc/attribution_ablation.hip and keep its contract: the occluded rows are a rule of
// the row-building skeleton (csrc/attribution_rows.h; scalar form only), the accumulation a memory-bound grid-stride loop, both
// tiny next to the classifier forwards they serve; the sum of bin (b, f, t) adds diff[k][b] over the windows k = kf * Kt + kt that
// cover it sequentially in increasing k from 0.f and divides by their count, as Captum's total_attrib += diff * mask;
// weights += mask; total_attrib / weights does.  No prefix sums, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "addvisor_hip.h"
#include "attribution_rows.h"
#include "common.h"

namespace advh {

// The occluded rows (csrc/attribution_rows.h): row g = k * B + b is x[b] with the baseline inside window k (kf = k / Kt,
// kt = k % Kt); rows g >= Kf * Kt * B are padding.
struct Occlusion2dRule {
    advh_occlusion2d_desc c;
    __host__ __device__ long n() const { return (long)c.Fm * c.Tm; }
    struct Row {
        bool pad;
        long k;   // the window (meaningless for a padding row)
        const float *xr, *br;
    };
    __device__ __forceinline__ Row row(long g) const {
        const long k = g / c.B, b = g - k * c.B;
        return {g >= (long)c.Kf * c.Kt * c.B, k, c.x + b * n(), c.base + (c.base_rows == 1 ? 0L : b * n())};
    }
    __device__ __forceinline__ float one(const Row& w, long q) const {
        const int f = (int)(q / c.Tm), t = (int)(q - (long)f * c.Tm);
        bool in = false;
        if (!w.pad) {
            const int f0 = (int)(w.k / c.Kt) * c.sf, t0 = (int)(w.k % c.Kt) * c.st;
            in = (f >= f0) & (f < f0 + c.wf) & (t >= t0) & (t < t0 + c.wt);   // no short circuit: one straight-line test
        }
        return in ? w.br[q] : w.xr[q];
    }
};

// the windows covering coordinate p of an axis: [lo, hi]
__device__ __forceinline__ void covering(int p, int w, int s, int K, int& lo, int& hi) {
    lo = p < w ? 0 : (p - w + s) / s;                 // ceil((p - w + 1) / s)
    hi = min(K - 1, p / s);
}

// attr[b][f][t] = (sum over kf = kf_lo..kf_hi, kt = kt_lo..kt_hi of f0[b] - fk[(kf * Kt + kt) * B + b], increasing k) / count
__global__ __launch_bounds__(256) void occlusion2d_accumulate_kernel(advh_occlusion2d_desc c, const float* __restrict__ f0,
                                                                     const float* __restrict__ fk, float* __restrict__ attr) {
    const long n = (long)c.Fm * c.Tm, total = (long)c.B * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / n, q = i - b * n;
        const int f = (int)(q / c.Tm), t = (int)(q - (long)f * c.Tm);
        int fl, fh, tl, th;
        covering(f, c.wf, c.sf, c.Kf, fl, fh);
        covering(t, c.wt, c.st, c.Kt, tl, th);
        const float fb = f0[b];
        float acc = 0.f;
        for (int kf = fl; kf <= fh; ++kf)
            for (int kt = tl; kt <= th; ++kt) acc += fb - fk[((long)kf * c.Kt + kt) * c.B + b];
        attr[i] = __fdiv_rn(acc, (float)((fh - fl + 1) * (th - tl + 1)));
    }
}

// out[b][ib][is] = sum of attr[b][f][t] over the box f in [ib * bw, min((ib + 1) * bw, Fm)), t in [is * sw, min((is + 1) * sw, Tm)):
// one workgroup per box.  Thread i adds the elements i, i + 256, ... of the UNCROPPED bw x sw box in that order (a cropped-away
// element adds nothing), then one 256-leaf tree in LDS: the order of every addition is fixed by (bw, sw) alone.
__global__ __launch_bounds__(256) void tf_pool_kernel(const float* __restrict__ attr, int Fm, int Tm, int bw, int sw, int nb, int ns,
                                                      float* __restrict__ out) {
    __shared__ float part[256];
    const int tid = threadIdx.x;
    const long box = blockIdx.x;
    const int is = (int)(box % ns), ib = (int)((box / ns) % nb);
    const long b = box / ((long)ns * nb);
    const float* a = attr + b * (long)Fm * Tm;
    float acc = 0.f;
    for (long e = tid; e < (long)bw * sw; e += 256) {
        const int f = ib * bw + (int)(e / sw), t = is * sw + (int)(e % sw);
        if (f < Fm && t < Tm) acc += a[(long)f * Tm + t];
    }
    part[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[box] = part[0];
}

}  // namespace advh

using namespace advh;

static bool axis_ok(int n, int w, int s, int K) {
    if (n < 1 || w < 1 || s < 1 || w > n || (s > w && w < n)) return false;
    return K == (n - w + s - 1) / s + 1;
}

static bool occlusion2d_ok(const advh_occlusion2d_desc* d) {
    if (!d || !d->x || !d->base || d->B <= 0) return false;
    if (d->base_rows != 1 && d->base_rows != d->B) return false;
    if (!axis_ok(d->Fm, d->wf, d->sf, d->Kf) || !axis_ok(d->Tm, d->wt, d->st, d->Kt)) return false;
    return (long)d->Kf * d->Kt <= 0x7fffffffL / d->B;
}

extern "C" int advh_occlusion2d_points(const advh_occlusion2d_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream) {
    if (!occlusion2d_ok(d) || !out || row0 < 0 || rows < 0) return ADVH_EINVAL;
    return build_rows<false>(Occlusion2dRule{*d}, false, (long)row0, rows, out, (hipStream_t)stream);
}

extern "C" int advh_occlusion2d_accumulate(const advh_occlusion2d_desc* d, const float* f0, const float* fk, float* attr,
                                           advh_stream_t stream) {
    if (!occlusion2d_ok(d) || !f0 || !fk || !attr) return ADVH_EINVAL;
    hipLaunchKernelGGL(occlusion2d_accumulate_kernel, dim3(grid_for((long)d->B * d->Fm * d->Tm)), dim3(256), 0, (hipStream_t)stream, *d,
                       f0, fk, attr);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_tf_pool(const float* attr, int B, int Fm, int Tm, int bw, int sw, float* out, advh_stream_t stream) {
    if (!attr || !out || B <= 0 || Fm <= 0 || Tm <= 0 || bw <= 0 || sw <= 0) return ADVH_EINVAL;
    const int nb = (Fm + bw - 1) / bw, ns = (Tm + sw - 1) / sw;
    const long boxes = (long)B * nb * ns;
    if (boxes > 0x7fffffffL) return ADVH_EINVAL;
    hipLaunchKernelGGL(tf_pool_kernel, dim3((unsigned)boxes), dim3(256), 0, (hipStream_t)stream, attr, Fm, Tm, bw, sw, nb, ns, out);
    return ADVH_LAUNCH_CHECK();
}
