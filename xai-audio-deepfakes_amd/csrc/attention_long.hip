// Fused self-attention for clips of any length: softmax(Q K^T / sqrt(d)) V with the keys streamed through LDS in blocks of
// KB = NTB * 16 and an online softmax (running row maximum m and sum l in the log2 domain; O rescaled by alpha = 2^(m_old - m_new)
// when a block raises the maximum), the loop of attention_x3_stream_kernel (attention.hip).  The whole-clip kernels of
// attention.hip / attention_ragged.hip stop at T = 256 frames (5.1 s); this file has no such limit.
//
// Grid (heads, B, ceil(ceil(T / 16) / 8)), 512 threads: a workgroup owns ONE block of eight query tiles (128 queries, one tile per
// wavefront) of a (clip, head) and streams every key block once, so the work of a workgroup is bounded by 128 x T whatever T is
// and a long clip spreads over several workgroups instead of re-staging all keys once per round of eight tiles in one.
//
// Per-clip bound: frames == nullptr -> Tv = T; otherwise Tv = clamp(frames[b], 1, T).  T stays the row STRIDE of qkv and ctx;
// every bound a stage sees is Tv (staging zero-fill, the -inf key mask, the block count, the query clamp, the stores), so clip b
// computes what the kernel computes for its first Tv rows alone.  Rows >= Tv of qkv are never read for their value; rows
// Tv <= t < T of ctx are written as zeros in every plane by the workgroup whose query block holds them.  The clamp is in the
// kernel, so no content of `frames` can move an access out of [0, T).
//
//   instance <NTB, D, NP, TR>   operands  KB    dynamic LDS (K [KB][D] + V^T [D][KB + 64], NP planes)
//   <16,  32, 2, false>         split     256    73 728 B
//   <16,  64, 2, false>         split     256   147 456 B   head dims 40 .. 56
//   < 7, 128, 2, false>         split     112   147 456 B   (the budget of attention_x3_stream_kernel<7, 128>)
//   <16,  32, 1, false>         fp16      256    36 864 B
//   <16,  64, 1, false>         fp16      256    73 728 B
//   <16, 128, 1, false>         fp16      256   147 456 B
//   <16,  64, 2, true>          split     256   131 072 B   head dim 64 exactly: K and V row-major by the LDS DMA (stage_dma), V^T
//                                                           fragments by the transposing LDS read (read_v_tr), as attention_x3_tr_kernel;
//                                                           added because the register-staged <16, 64, 2> measured 0.74 of the
//                                                           whole-clip kernel's pair rate at 16 x 499 x 12 x 64
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "attention_tiles.h"

namespace advh {

// K [KB][D] and V^T [D][KB + 64] of one key block in NP planes: att_x3_lds' formula of attention.hip, halved for one plane.
// TR: K and V row-major, no skew (att_x3_tr_lds' formula).
constexpr size_t att_long_lds(int ntb, int D, int np, bool tr) {
    return tr ? (size_t)np * 2 * ntb * 16 * D * 2 : (size_t)np * (ntb * 16 * D + D * (ntb * 16 + 64)) * 2;
}

template <bool TR, int NTB, int D>
__device__ __forceinline__ auto long_read_v(_Float16* Vt, int lane, int fr, int g) {
    if constexpr (TR) return read_v_tr<NTB>{(const __attribute__((address_space(3))) char*)LDS_PTR(Vt), lane};
    else return read_v_t<NTB, D>{Vt, fr, g};
}

template <int NTB, int D, int NP, bool TR>
__global__ __launch_bounds__(512, 1) void attention_long_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                long ctx_lo, const int* __restrict__ frames, int T, int H, int dm,
                                                                float scale) {
    constexpr int KB = NTB * 16, VP = KB + 64, NS = (NTB + 1) / 2, KK = D / 32, DT = D / 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    static_assert(!TR || D == 64, "the DMA staging and the transposing read are written for 128-byte rows");
    _Float16* Ks = att_lds;                      // [NP][KB * D]
    _Float16* Vt = att_lds + NP * KB * D;        // [NP][D * VP]; TR: V row-major, [NP][KB * D]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * 128;        // row0 < T: the grid has ceil(T / 128) blocks
    int Tv = T;
    if (frames) {
        const int f = frames[b];
        Tv = f < 1 ? 1 : (f > T ? T : f);
    }
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    _Float16* cb = ctx + (long)b * T * H + head * dm;

    // rows max(Tv, row0) <= t < min(T, row0 + 128) of this head's dm columns <- 0, every plane (dm % 8 == 0: 8-byte stores at
    // the columns store_ctx writes).  First: no later stage touches these rows.
    {
        const int z0 = Tv > row0 ? Tv : row0, z1 = T < row0 + 128 ? T : row0 + 128, c4 = dm / 4, n = (z1 - z0) * c4;
        for (int i = tid; i < n; i += 512) {
            const long o = (long)(z0 + i / c4) * H + (i % c4) * 4;
#pragma unroll
            for (int p = 0; p < NP; ++p) *(f16x4*)(cb + p * ctx_lo + o) = f16x4{0, 0, 0, 0};
        }
    }
    if (row0 >= Tv) return;                      // workgroup-uniform, before any barrier

    const int nblk = (Tv + KB - 1) / KB;
    const auto read_v = long_read_v<TR, NTB, D>(Vt, lane, fr, g);
    const int qt = blockIdx.z * 8 + wv;
    const bool live = qt * 16 < Tv;              // wave-uniform; idle wavefronts still take part in staging and barriers
    const int qrow = qt * 16 + fr;
    const int qr = qrow < Tv ? qrow : Tv - 1;
    f16x8 q[KK][NP];
    load_q<KK, NP>(q, base, qkv_lo, (long)qr * ld, g, dm / 8, live);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o[DT][NP];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int p = 0; p < NP; ++p) o[dt][p] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int blk = 0; blk < nblk; ++blk) {
        const int k0 = blk * KB;
        __syncthreads();                         // every wavefront is done with the previous block
        if constexpr (TR) {                      // the block's rows from k0 on; keys >= Tv re-read key Tv - 1 (masked below, P = 0)
            stage_dma<KB, 512, NP>((char*)Ks, (char*)Vt, base + (long)k0 * ld, qkv_lo, ld, H, Tv - k0, tid);
        } else {
#pragma unroll 1
            for (int pl = 0; pl < 2 * NP; ++pl) {    // K planes, then V planes: one tensor plane at a time (staging registers)
                const bool isv = pl >= NP;
                const int p = pl % NP;
                stage_regs<KB, D, 512, 1>(Ks + p * KB * D, Vt + p * D * VP, base + (p ? qkv_lo : 0) + (isv ? 2 * H : H), 0, isv, ld, dm / 8, Tv,
                                          k0, tid);
            }
        }
        __syncthreads();
        if (!live) continue;
        f32x4 s[NTB];
        score_tiles<NTB, D, NP>(s, Ks, q, fr, g);
        const float mx = mask_scale_max<NTB>(s, scale, k0, Tv, g);
        const float m_new = fmaxf(m_run, mx);     // finite: every block holds at least one key < Tv
        const float alpha = NP == 1 ? __builtin_amdgcn_exp2f(m_run - m_new) : exp2f(m_run - m_new);   // 0 for the first block (m_run = -inf)
        l_run = l_run * alpha + exp_sum<NTB, NP == 1>(s, m_new);
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][p][r] *= alpha;
        // un-normalised probabilities (<= 1) as the B operand, built per 32-key step right before its MFMAs (register budget, as
        // in attention_x3_stream_kernel); the 1 / l normalisation happens once at the end
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
            f16x8 p[NP];
            pack_p<NTB, NP, false>(p, s, ss, 1.f);
            pv_step<DT, NP>(o, p, ss, read_v);
        }
    }
    if (live && qrow < Tv) {
        const float inv = 1.f / l_run;
        if constexpr (NP == 1) {                 // store_ctx normalises the joined planes only: one plane is scaled here
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][0][r] *= inv;
        }
        store_ctx<DT, NP, true>(cb, ctx_lo, (long)qrow * H, o, g, dm, inv);
    }
}

}  // namespace advh

using namespace advh;

// Raise the dynamic-LDS limit of every instance (advh_init).
int advh_init_attention_long() {
#define RAISE(NTB_, D_, NP_, TR_)                                                                                                   \
    if (hipFuncSetAttribute((const void*)attention_long_kernel<NTB_, D_, NP_, TR_>, hipFuncAttributeMaxDynamicSharedMemorySize,     \
                            (int)att_long_lds(NTB_, D_, NP_, TR_)) != hipSuccess) return ADVH_ELAUNCH;
    RAISE(16, 32, 2, false) RAISE(16, 64, 2, false) RAISE(7, 128, 2, false) RAISE(16, 32, 1, false) RAISE(16, 64, 1, false)
    RAISE(16, 128, 1, false) RAISE(16, 64, 2, true)
#undef RAISE
    return ADVH_OK;
}

// The limits both entries share, decided before any launch: head dim, and the grid's y and z extents.
static int long_unsupported(int B, int T, int dm) {
    const long nqb = ((long)T + 127) / 128;
    return dm % 8 || dm > 128 || B > 65535 || nqb > 65535;
}

template <int NTB, int D, int NP, bool TR = false>
static void launch_long(const _Float16* q, long ql, _Float16* c, long cl, const int* fv, int B, int T, int H, int heads, int dm, hipStream_t s) {
    const dim3 grid(heads, B, (T + 127) / 128), block(512);
    hipLaunchKernelGGL((attention_long_kernel<NTB, D, NP, TR>), grid, block, att_long_lds(NTB, D, NP, TR), s, q, ql, c, cl, fv, T, H, dm,
                       1.f / sqrtf((float)dm));
}

extern "C" int advh_attention_long_f16(const void* qkv, void* ctx, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    const int dm = H / heads;
    if (long_unsupported(B, T, dm)) return ADVH_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    const int* fv = (const int*)frames;
    if (dm <= 32) launch_long<16, 32, 1>(q, 0, c, 0, fv, B, T, H, heads, dm, s);
    else if (dm <= 64) launch_long<16, 64, 1>(q, 0, c, 0, fv, B, T, H, heads, dm, s);
    else launch_long<16, 128, 1>(q, 0, c, 0, fv, B, T, H, heads, dm, s);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_attention_long_split(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, const int32_t* frames, int B, int T, int H,
                                         int heads, advh_stream_t stream) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads || qkv_lo <= 0 || ctx_lo <= 0 || qkv_lo % 8 || ctx_lo % 4)
        return ADVH_EINVAL;
    const int dm = H / heads;
    if (long_unsupported(B, T, dm)) return ADVH_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    const int* fv = (const int*)frames;
    const long ql = (long)qkv_lo, cl = (long)ctx_lo;
    if (dm <= 32) launch_long<16, 32, 2>(q, ql, c, cl, fv, B, T, H, heads, dm, s);
    else if (dm == 64) launch_long<16, 64, 2, true>(q, ql, c, cl, fv, B, T, H, heads, dm, s);      // DMA staging + transposing V^T reads
    else if (dm <= 64) launch_long<16, 64, 2>(q, ql, c, cl, fv, B, T, H, heads, dm, s);
    else launch_long<7, 128, 2>(q, ql, c, cl, fv, B, T, H, heads, dm, s);      // keys in blocks of 112
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention_long)
