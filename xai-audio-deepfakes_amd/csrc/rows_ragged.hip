// Row kernels of the ragged embedder forward: zeroing the padded rows of the hidden states and the time-pool + logistic head
// over each clip's valid frames.  frames: int32 [B] on the device, clip b has frames[b] valid rows of its T.
//
// HF zeroes padded rows after the feature projection (Wav2Vec2Encoder / Wav2Vec2EncoderStableLayerNorm .forward,
// modeling_wav2vec2.py: hidden_states[~expand_attention_mask] = 0), so the positional convolution of a valid frame sees the
// zero padding it would see in the clip run alone; advh_zero_tail_rows is that statement, and also clears the returned hidden
// states.  The pool kernels are the text of rowops.hip's with the clip base kept at b * T rows and the frame loop / divisor
// taken from frames[b]: the valid frames are added in the batch form's order, so frames[b] = T reproduces it bit for bit.  (The
// kernels of rowops.hip are left exactly as they are; sharing one inlined body changed their code.)
#include <hip/hip_runtime.h>
#include "addvisor_hip.h"
#include "common.h"

namespace advh {
namespace ragged {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// frames[b] clamped to [lo, T]: no content of `frames` moves an access out of clip b's T rows
__device__ __forceinline__ int clip_frames(const int* __restrict__ frames, int b, int lo, int T) {
    const int f = frames[b];
    return f < lo ? lo : (f > T ? T : f);
}

// x[b, frames[b]:, :] = 0.  Grid row b = clip b.  VEC: 16-byte stores (x 16-byte aligned and H % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void zero_tail_rows_kernel(float* __restrict__ x, const int* __restrict__ frames, int T, int H) {
    const int b = blockIdx.y, f0 = clip_frames(frames, b, 0, T);
    float* xb = x + ((long)b * T + f0) * H;
    const long n = (long)(T - f0) * H;
    const long start = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (VEC) {
        for (long i = start; i < n / 4; i += step) ((float4*)xb)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (long i = start; i < n; i += step) xb[i] = 0.f;
    }
}

// logit[b] = mean_{t < Tv}(h[b,t,:]) . coef + intercept;  prob = sigmoid(logit).  Fast path (H % 4 == 0, H <= 2048).
template <int NV>
__global__ __launch_bounds__(256) void pool_logreg_rows_ragged_kernel(const float* __restrict__ h, const float* __restrict__ coef,
                                                                      float intercept, float* __restrict__ logit,
                                                                      float* __restrict__ prob, float* __restrict__ pooled,
                                                                      const int* __restrict__ frames, int Ts, int H) {
    extern __shared__ float part[];                       // [4][H]
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = clip_frames(frames, b, 1, Ts);
    const float* hb = h + (long)b * Ts * H;
    float4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = wv; t < T; t += 8) {
        const bool two = t + 4 < T;
        float4 a[NV], c2[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = 4 * (lane + 64 * i);
            a[i] = c < H ? *(const float4*)(hb + (long)t * H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            c2[i] = (two && c < H) ? *(const float4*)(hb + (long)(t + 4) * H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            acc[i].x += a[i].x; acc[i].y += a[i].y; acc[i].z += a[i].z; acc[i].w += a[i].w;
            acc[i].x += c2[i].x; acc[i].y += c2[i].y; acc[i].z += c2[i].z; acc[i].w += c2[i].w;
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * (lane + 64 * i);
        if (c < H) *(float4*)(part + wv * H + c) = acc[i];
    }
    __syncthreads();
    float dot = 0.f;
    for (int c = tid; c < H; c += 256) {
        const float s = ((part[c] + part[H + c]) + (part[2 * H + c] + part[3 * H + c])) / T;
        if (pooled) pooled[(long)b * H + c] = s;
        dot += s * coef[c];
    }
    dot = wave_sum(dot);
    if (lane == 0) red[wv] = dot;
    __syncthreads();
    if (tid == 0) {
        float z = (red[0] + red[1]) + (red[2] + red[3]) + intercept;
        logit[b] = z;
        prob[b] = 1.f / (1.f + expf(-z));
    }
}

// any H: one thread per channel, frames in order
__global__ __launch_bounds__(256) void pool_logreg_ragged_kernel(const float* __restrict__ h, const float* __restrict__ coef,
                                                                 float intercept, float* __restrict__ logit,
                                                                 float* __restrict__ prob, float* __restrict__ pooled,
                                                                 const int* __restrict__ frames, int Ts, int H) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = clip_frames(frames, b, 1, Ts);
    const float* hb = h + (long)b * Ts * H;
    float dot = 0.f;
    for (int c = tid; c < H; c += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += hb[(long)t * H + c];
        s /= T;
        if (pooled) pooled[(long)b * H + c] = s;
        dot += s * coef[c];
    }
    dot = wave_sum(dot);
    if ((tid & 63) == 0) red[tid >> 6] = dot;
    __syncthreads();
    if (tid == 0) {
        float z = (red[0] + red[1]) + (red[2] + red[3]) + intercept;
        logit[b] = z;
        prob[b] = 1.f / (1.f + expf(-z));
    }
}

}  // namespace ragged
}  // namespace advh

using namespace advh::ragged;

extern "C" int advh_zero_tail_rows(float* x, const int32_t* frames, int B, int T, int H, advh_stream_t stream) {
    if (!x || !frames || B <= 0 || T <= 0 || H <= 0) return ADVH_EINVAL;
    if (B > 65535) return ADVH_EUNSUPPORTED;                 // one grid row per clip
    const bool vec = aligned16(x) && H % 4 == 0;
    const dim3 grid(grid_for((long)T * H / (vec ? 4 : 1), 64), B);
    launch_vec(vec, zero_tail_rows_kernel<true>, zero_tail_rows_kernel<false>, grid, (hipStream_t)stream, x, (const int*)frames, T, H);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_pool_logreg_ragged(const float* h, const float* coef, float intercept, float* logit, float* prob,
                                       float* pooled, const int32_t* frames, int B, int T, int H, advh_stream_t stream) {
    if (!h || !coef || !logit || !prob || !frames || B <= 0 || T <= 0 || H <= 0) return ADVH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int* fv = (const int*)frames;
    const size_t lds = 4 * (size_t)H * sizeof(float);
    if (H % 4 == 0 && H <= 1024)
        hipLaunchKernelGGL(pool_logreg_rows_ragged_kernel<4>, dim3(B), dim3(256), lds, s, h, coef, intercept, logit, prob, pooled, fv, T, H);
    else if (H % 4 == 0 && H <= 2048)
        hipLaunchKernelGGL(pool_logreg_rows_ragged_kernel<8>, dim3(B), dim3(256), lds, s, h, coef, intercept, logit, prob, pooled, fv, T, H);
    else
        hipLaunchKernelGGL(pool_logreg_ragged_kernel, dim3(B), dim3(256), 0, s, h, coef, intercept, logit, prob, pooled, fv, T, H);
    return ADVH_LAUNCH_CHECK();
}
