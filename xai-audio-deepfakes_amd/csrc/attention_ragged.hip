// Fused self-attention over a ragged batch: clip b of a [B][T] row layout has frames[b] valid frames, the rest is padding.
// HF masks padded KEYS with an additive -inf in front of the softmax (modeling_wav2vec2.py, Wav2Vec2Encoder.forward: the
// attention_mask expanded to [B, 1, T, T]) and zeroes padded rows of the hidden states (hidden_states[~expand_attention_mask] = 0).
// Here the mask is the validity bound every stage of attention_tiles.h already takes: each kernel below is its sibling of
// attention.hip with
//     T   kept as the row STRIDE of qkv and ctx (b * T * ld, b * T * H), and
//     Tv  = clamp(frames[b], 1, T) passed wherever a stage takes its bound (staging, key mask, query clamp, tile loops),
// so clip b computes exactly what the sibling computes for its first Tv rows alone.  Rows >= Tv of qkv are never read for
// their value (register staging leaves them zero, the DMA staging re-reads key Tv - 1, query rows clamp to Tv - 1) and rows
// Tv <= t < T of ctx are written as zeros in both planes: ctx comes from an uninitialised allocation and feeds the
// out-projection, whose split conversion would raise the range flag on a stale value.  The clamp is in the kernel, so no content
// of `frames` can move an access out of [0, T); frames[b] is one scalar load per workgroup (b = blockIdx.y is uniform).
//
//   kernel                              sibling (attention.hip)        LDS / launch bounds: the sibling's
//   attention_ragged_kernel             attention_kernel               D = 128 composed from the stages like D < 128
//   attention_ragged_tr_kernel          attention_tr_kernel
//   attention_ragged_x3_kernel          attention_x3_kernel
//   attention_ragged_x3_tr_kernel       attention_x3_tr_kernel
//   attention_ragged_x3_stream_kernel   attention_x3_stream_kernel
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "attention_tiles.h"

namespace advh {

__device__ __forceinline__ int valid_frames(const int* __restrict__ frames, int b, int T) {
    const int f = frames[b];
    return f < 1 ? 1 : (f > T ? T : f);
}

// Rows Tv <= t < T of this (clip, head)'s dm columns <- 0, every plane.  ctx points at the (clip, head)'s first row; dm % 8 == 0
// and the sibling's own stores are 8-byte vectors at the same columns, so these are aligned wherever those are.  Every kernel
// calls it FIRST: no later stage touches these rows, and T and the loop's registers are dead before the staging begins (called
// last it cost 1 - 5 VGPRs and one occupancy step in two instances; first, every instance keeps its sibling's VGPR count and
// occupancy, attention_ragged_x3_kernel<13, 64> within one register).
template <int NTH, int NP>
__device__ __forceinline__ void zero_tail(_Float16* ctx, long ctx_lo, int H, int Tv, int T, int dm, int tid) {
    const int c4 = dm / 4, n = (T - Tv) * c4;
    for (int i = tid; i < n; i += NTH) {
        const long o = (long)(Tv + i / c4) * H + (i % c4) * 4;
#pragma unroll
        for (int p = 0; p < NP; ++p) *(f16x4*)(ctx + p * ctx_lo + o) = f16x4{0, 0, 0, 0};
    }
}

template <int NT, int D>
__global__ __launch_bounds__(256, (D <= 64 ? 2 : 1)) void attention_ragged_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                                                   const int* __restrict__ frames, int T, int H, int dm, float scale) {
    constexpr int NKEY = NT * 16, VP = NKEY + 64;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[NKEY * D];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[D * VP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Tv = valid_frames(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    _Float16* cb = ctx + (long)b * T * H + head * dm;
    zero_tail<256, 1>(cb, 0, H, Tv, T, dm, tid);
    stage_regs<NKEY, D, 256, 2>(Ks, Vt, base + H, H, false, ld, dm / 8, Tv, 0, tid);
    __syncthreads();
    const read_v_t<NT, D> read_v{Vt, fr, g};
    for (int qt = wv; qt * 16 < Tv; qt += 4)
        attend_tile<NT, D, 1>(base, 0, ld, Ks, read_v, cb, 0, H, Tv, dm, scale, qt, fr, g);
}

template <int NT>
__global__ __launch_bounds__(256, 2) void attention_ragged_tr_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                                     const int* __restrict__ frames, int T, int H, float scale) {
    constexpr int D = 64, NKEY = NT * 16;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[NKEY * D];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[NKEY * D];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Tv = valid_frames(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * D;
    _Float16* cb = ctx + (long)b * T * H + head * D;
    zero_tail<256, 1>(cb, 0, H, Tv, T, D, tid);
    stage_dma<NKEY, 256, 1>((char*)Ks, (char*)Vs, base, 0, ld, H, Tv, tid);
    __syncthreads();
    const read_v_tr<NT> read_v{(const __attribute__((address_space(3))) char*)LDS_PTR(Vs), lane};
    for (int qt = wv; qt * 16 < Tv; qt += 4)
        attend_tile<NT, D, 1>(base, 0, ld, Ks, read_v, cb, 0, H, Tv, D, scale, qt, fr, g);
}

// Dynamic LDS: the figures of attention.hip's split instances.
constexpr size_t att_x3_lds(int nt, int D) { return (size_t)2 * (nt * 16 * D + D * (nt * 16 + 64)) * 2; }
constexpr size_t att_x3_tr_lds(int nt) { return (size_t)4 * nt * 16 * 64 * 2; }

template <int NT, int D>
__global__ __launch_bounds__(512, 1) void attention_ragged_x3_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                     long ctx_lo, const int* __restrict__ frames, int T, int H, int dm, float scale) {
    constexpr int NKEY = NT * 16, VP = NKEY + 64;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2][NKEY * D]
    _Float16* Vt = att_lds + 2 * NKEY * D;       // [2][D * VP]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Tv = valid_frames(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    _Float16* cb = ctx + (long)b * T * H + head * dm;
    zero_tail<512, 2>(cb, ctx_lo, H, Tv, T, dm, tid);
    for (int pl = 0; pl < 2; ++pl)
        stage_regs<NKEY, D, 512, 2>(Ks + pl * NKEY * D, Vt + pl * D * VP, base + (pl ? qkv_lo : 0) + H, H, false, ld, dm / 8, Tv, 0, tid);
    __syncthreads();
    const read_v_t<NT, D> read_v{Vt, fr, g};
    for (int qt = wv; qt * 16 < Tv; qt += 8)
        attend_tile<NT, D, 2>(base, qkv_lo, ld, Ks, read_v, cb, ctx_lo, H, Tv, dm, scale, qt, fr, g);
}

// Keys streamed in blocks with an online softmax (head dims 72 .. 128): nqt and nblk follow Tv, so every block that is staged
// holds at least one valid key and the running maximum stays finite.
template <int NTB, int D>
__global__ __launch_bounds__(512, 1) void attention_ragged_x3_stream_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                            long ctx_lo, const int* __restrict__ frames, int T, int H, int dm,
                                                                            float scale) {
    constexpr int KB = NTB * 16, VP = KB + 64, NS = (NTB + 1) / 2, KK = D / 32, DT = D / 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2][KB * D]
    _Float16* Vt = att_lds + 2 * KB * D;         // [2][D * VP]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Tv = valid_frames(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    _Float16* cb = ctx + (long)b * T * H + head * dm;
    zero_tail<512, 2>(cb, ctx_lo, H, Tv, T, dm, tid);
    const int nqt = (Tv + 15) / 16, nblk = (Tv + KB - 1) / KB;
    const read_v_t<NTB, D> read_v{Vt, fr, g};

    for (int q0 = 0; q0 < nqt; q0 += 8) {
        const int qt = q0 + wv;
        const bool live = qt < nqt;                  // wave-uniform; idle wavefronts still take part in staging and barriers
        const int qrow = qt * 16 + fr;
        const int qr = qrow < Tv ? qrow : Tv - 1;
        f16x8 q[KK][2];
        load_q<KK, 2>(q, base, qkv_lo, (long)qr * ld, g, dm / 8, live);
        float m_run = -INFINITY, l_run = 0.f;
        f32x4 o[DT][2];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) { o[dt][0] = f32x4{0.f, 0.f, 0.f, 0.f}; o[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

        for (int blk = 0; blk < nblk; ++blk) {
            const int k0 = blk * KB;
            __syncthreads();                         // every wavefront is done with the previous block
#pragma unroll 1
            for (int pl = 0; pl < 4; ++pl) {         // K hi, K lo, V hi, V lo: one tensor plane at a time (staging registers)
                const bool isv = pl >= 2;
                stage_regs<KB, D, 512, 1>(Ks + (pl & 1) * KB * D, Vt + (pl & 1) * D * VP, base + ((pl & 1) ? qkv_lo : 0) + (isv ? 2 * H : H), 0,
                                          isv, ld, dm / 8, Tv, k0, tid);
            }
            __syncthreads();
            if (!live) continue;
            f32x4 s[NTB];
            score_tiles<NTB, D, 2>(s, Ks, q, fr, g);
            const float mx = mask_scale_max<NTB>(s, scale, k0, Tv, g);
            const float m_new = fmaxf(m_run, mx);     // finite: every block holds at least one key < Tv
            const float alpha = exp2f(m_run - m_new); // 0 for the first block (m_run = -inf)
            l_run = l_run * alpha + exp_sum<NTB, false>(s, m_new);
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[dt][0][r] *= alpha; o[dt][1][r] *= alpha; }
#pragma unroll
            for (int ss = 0; ss < NS; ++ss) {        // P per 32-key step right before its MFMAs, as in the sibling (register budget)
                f16x8 p[2];
                pack_p<NTB, 2, false>(p, s, ss, 1.f);
                pv_step<DT, 2>(o, p, ss, read_v);
            }
        }
        if (live && qrow < Tv) store_ctx<DT, 2, true>(cb, ctx_lo, (long)qrow * H, o, g, dm, 1.f / l_run);
    }
}

template <int NT>
__global__ __launch_bounds__(512, 1) void attention_ragged_x3_tr_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                        long ctx_lo, const int* __restrict__ frames, int T, int H, float scale) {
    constexpr int D = 64, NKEY = NT * 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2 planes][NKEY][64]
    _Float16* Vs = att_lds + 2 * NKEY * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Tv = valid_frames(frames, b, T);
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * D;
    _Float16* cb = ctx + (long)b * T * H + head * D;
    zero_tail<512, 2>(cb, ctx_lo, H, Tv, T, D, tid);
    stage_dma<NKEY, 512, 2>((char*)Ks, (char*)Vs, base, qkv_lo, ld, H, Tv, tid);
    __syncthreads();
    const read_v_tr<NT> read_v{(const __attribute__((address_space(3))) char*)LDS_PTR(Vs), lane};
    for (int qt = wv; qt * 16 < Tv; qt += 8)
        attend_tile<NT, D, 2>(base, qkv_lo, ld, Ks, read_v, cb, ctx_lo, H, Tv, D, scale, qt, fr, g);
}

}  // namespace advh

using namespace advh;

// f(NT) with the tile-count class NT of nt = ceil(T / 16) <= 16 key tiles: the classes of attention.hip, chosen by the row
// stride T (the lengths live on the device; Tv <= T fits every class T fits).
template <class F>
static void with_tile_class(int nt, F&& f) {
    if (nt <= 4) f(std::integral_constant<int, 4>{});
    else if (nt <= 8) f(std::integral_constant<int, 8>{});
    else if (nt <= 13) f(std::integral_constant<int, 13>{});
    else f(std::integral_constant<int, 16>{});
}

extern "C" int advh_attention_f16_ragged(const void* qkv, void* ctx, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !ctx || !frames || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const float scale = 1.f / sqrtf((float)dm);
    const dim3 grid(heads, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    const int* fv = (const int*)frames;
    with_tile_class((T + 15) / 16, [&](auto cls) {
        constexpr int NT = decltype(cls)::value;
        if (dm == 64) hipLaunchKernelGGL((attention_ragged_tr_kernel<NT>), grid, block, 0, s, q, c, fv, T, H, scale);
        else if (dm <= 32) hipLaunchKernelGGL((attention_ragged_kernel<NT, 32>), grid, block, 0, s, q, c, fv, T, H, dm, scale);
        else if (dm <= 64) hipLaunchKernelGGL((attention_ragged_kernel<NT, 64>), grid, block, 0, s, q, c, fv, T, H, dm, scale);
        else hipLaunchKernelGGL((attention_ragged_kernel<(NT == 8 ? 13 : NT), 128>), grid, block, 0, s, q, c, fv, T, H, dm, scale);   // no 8 class at D = 128
    });
    return ADVH_LAUNCH_CHECK();
}

// Raise the dynamic-LDS limit of the ragged split instances (advh_init).
int advh_init_attention_ragged() {
#define RAISE(kernel, bytes)                                                                                                        \
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) != hipSuccess) return ADVH_ELAUNCH;
#define X3(NT_) RAISE((attention_ragged_x3_kernel<NT_, 32>), att_x3_lds(NT_, 32)) RAISE((attention_ragged_x3_kernel<NT_, 64>), att_x3_lds(NT_, 64)) \
                RAISE(attention_ragged_x3_tr_kernel<NT_>, att_x3_tr_lds(NT_))
    X3(4) X3(8) X3(13) X3(16)
    RAISE((attention_ragged_x3_stream_kernel<7, 128>), att_x3_lds(7, 128))
#undef X3
#undef RAISE
    return ADVH_OK;
}

extern "C" int advh_attention_split_ragged(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, const int32_t* frames, int B, int T, int H,
                                           int heads, advh_stream_t stream) {
    if (!qkv || !ctx || !frames || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads || qkv_lo <= 0 || ctx_lo <= 0 || qkv_lo % 8 || ctx_lo % 4)
        return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const float scale = 1.f / sqrtf((float)dm);
    const dim3 grid(heads, B), block(512);
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    const int* fv = (const int*)frames;
    const long ql = (long)qkv_lo, cl = (long)ctx_lo;
    if (dm > 64)                                         // keys streamed in blocks of 112 with an online softmax
        hipLaunchKernelGGL((attention_ragged_x3_stream_kernel<7, 128>), grid, block, att_x3_lds(7, 128), s, q, ql, c, cl, fv, T, H, dm, scale);
    else with_tile_class((T + 15) / 16, [&](auto cls) {
        constexpr int NT = decltype(cls)::value;
        if (dm == 64) hipLaunchKernelGGL((attention_ragged_x3_tr_kernel<NT>), grid, block, att_x3_tr_lds(NT), s, q, ql, c, cl, fv, T, H, scale);
        else if (dm <= 32) hipLaunchKernelGGL((attention_ragged_x3_kernel<NT, 32>), grid, block, att_x3_lds(NT, 32), s, q, ql, c, cl, fv, T, H, dm, scale);
        else hipLaunchKernelGGL((attention_ragged_x3_kernel<NT, 64>), grid, block, att_x3_lds(NT, 64), s, q, ql, c, cl, fv, T, H, dm, scale);
    });
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention_ragged)
