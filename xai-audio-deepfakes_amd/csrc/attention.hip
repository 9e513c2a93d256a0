// Fused self-attention for short sequences (T <= 256): softmax(Q K^T / sqrt(d)) V, no mask
// (transformers/.../modeling_wav2vec2.py:438-548; the reference forces the math SDP path,
// train_addvisor.py:21-23).  wav2vec2 sees T = 199 frames for a 4 s clip (249 for 5 s), so the whole
// K and V of one (clip, head) fit in LDS and the softmax is single-pass: no online rescaling -- except in the fp32-class
// format at head dims above 64, where the keys stream through LDS in blocks.
//
// One workgroup per (head, clip); each of its wavefronts owns 16-query tiles.  The stages live in attention_tiles.h; the five
// kernels below differ in how K and V reach LDS and in the operand format:
//
//   kernel                       operands  K / V staging               V^T fragments     query tiles
//   attention_kernel             fp16      registers, V transposed     read_v_t          attend_tile (single pass); D = 128: own body
//   attention_tr_kernel          fp16      LDS DMA, row-major (dm 64)  read_v_tr         attend_tile
//   attention_x3_kernel          split     registers, V transposed     read_v_t          attend_tile
//   attention_x3_tr_kernel       split     LDS DMA, row-major (dm 64)  read_v_tr         attend_tile
//   attention_x3_stream_kernel   split     registers, per key block    read_v_t          its own loop: online softmax
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "attention_tiles.h"

namespace advh {

// dm = the real head dim (a multiple of 8): chunks beyond it are zero-filled on load and skipped on store
// (XLS-R-2B: 1920 / 16 heads = 120 -> D = 128).
template <int NT, int D>
__global__ __launch_bounds__(256, (D <= 64 ? 2 : 1)) void attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                        int T, int H, int dm, float scale) {
    constexpr int NKEY = NT * 16, CH = D / 8, VP = NKEY + 64 /* row pitch incl. the per-8-rows skew that spreads the transposing stores over the banks */, NS = (NT + 1) / 2, KK = D / 32, DT = D / 16;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[NKEY * D];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[D * VP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    const int chm = dm / 8;                          // real 16-byte chunks per row
    if constexpr (D < 128) {
        const int fr = lane & 15, g = lane >> 4;
        stage_regs<NKEY, D, 256, 2>(Ks, Vt, base + H, H, false, ld, chm, T, 0, tid);
        __syncthreads();
        const read_v_t<NT, D> read_v{Vt, fr, g};
        for (int qt = wv; qt * 16 < T; qt += 4)
            attend_tile<NT, D, 1>(base, 0, ld, Ks, read_v, ctx + (long)b * T * H + head * dm, 0, H, T, dm, scale, qt, fr, g);
    } else {
        // D = 128 keeps the body it had before the stages were folded, stage for stage the same steps as attend_tile.  Composed from
        // attention_tiles.h, attention_kernel<13,128> measured 0.6 - 0.7 us of 120 us (0.5 %) slower at 64 x 199 x 16 x 120, twice,
        // outside the 0.3 - 0.5 us the previous build differs from itself; no single stage could be named as the cause (swapping any
        // one stage of this body for its folded form reorders the whole kernel's schedule).  This text compiles to the previous
        // build's code instruction for instruction for all three D = 128 instances.  Fold it when a composition measures level.
        // ---- stage K (row-major, 16-byte chunks XOR-swizzled by row) and V^T; keys >= T are zero
        // all global loads of this thread are issued before the first LDS store: one memory latency per workgroup instead
        // of one per loop iteration (the transposing stores are scalar and would otherwise serialise behind each load)
        constexpr int NIT = (NKEY * CH + 255) / 256;
        f16x8 kreg[NIT], vreg[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * 256, key = i / CH, c = i % CH;
            kreg[it] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            vreg[it] = kreg[it];
            if (i < NKEY * CH && key < T && c < chm) {
                kreg[it] = *(const f16x8*)(base + (long)key * ld + H + c * 8);
                vreg[it] = *(const f16x8*)(base + (long)key * ld + 2 * H + c * 8);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * 256, key = i / CH, c = i % CH;
            if (i >= NKEY * CH) break;
            *(f16x8*)(Ks + key * D + ((c ^ (key & (CH - 1))) * 8)) = kreg[it];
#pragma unroll
            for (int j = 0; j < 8; ++j) Vt[(c * 8 + j) * VP + (c & 7) * 8 + key] = vreg[it][j];
        }
        __syncthreads();

        const int fr = lane & 15, g = lane >> 4;
        for (int qt = wv; qt * 16 < T; qt += 4) {
            int qrow = qt * 16 + fr;
            int qr = qrow < T ? qrow : T - 1;
            f16x8 qf[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                qf[kk] = (kk * 4 + g < chm) ? *(const f16x8*)(base + (long)qr * ld + kk * 32 + g * 8) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};

            // S^T tiles: rows = keys (4g + r within the tile), column = this lane's query
            f32x4 s[NT];
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    int key = kt * 16 + fr, c = kk * 4 + g;
                    f16x8 kf = *(const f16x8*)(Ks + key * D + ((c ^ (key & (CH - 1))) * 8));
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[kk], s[kt], 0, 0, 0);
                }
                if ((kt & 1) == 1) __builtin_amdgcn_sched_barrier(0);       // keep the K-fragment reads from being hoisted en bloc (VGPR pressure)
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = (kt * 16 + g * 4 + r < T) ? s[kt][r] * (scale * LOG2E) : -INFINITY;   // log2 domain: exp(x) = v_exp_f32(x log2 e)
                    s[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { float e = __builtin_amdgcn_exp2f(s[kt][r] - mx); s[kt][r] = e; sum += e; }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.f / sum;

            // P as the B operand of each 32-key step: elements 0-3 from tile 2s, 4-7 from tile 2s+1
            f16x8 pf[NS];
#pragma unroll
            for (int ss = 0; ss < NS; ++ss) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pf[ss][r] = (_Float16)(s[2 * ss][r] * inv);
                    pf[ss][4 + r] = (2 * ss + 1 < NT) ? (_Float16)(s[(2 * ss + 1 < NT) ? 2 * ss + 1 : 0][r] * inv) : (_Float16)0.f;
                }
            }
            // O^T = V^T P^T, key steps outermost so only one step's V^T fragments are live at a time
            f32x4 o[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ss = 0; ss < NS; ++ss) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const _Float16* vr = Vt + (dt * 16 + fr) * VP + (((dt * 16 + fr) >> 3) & 7) * 8 + ss * 32 + g * 4;
                    f16x4 lo = *(const f16x4*)vr;
                    f16x4 hi = (2 * ss + 1 < NT) ? *(const f16x4*)(vr + 16) : f16x4{0, 0, 0, 0};
                    f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[ss], o[dt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (qrow < T) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    if (dt * 16 + g * 4 >= dm) continue;
                    f16x4 hv = {(_Float16)o[dt][0], (_Float16)o[dt][1], (_Float16)o[dt][2], (_Float16)o[dt][3]};
                    *(f16x4*)(ctx + ((long)b * T + qrow) * H + head * dm + dt * 16 + g * 4) = hv;
                }
            }
        }
    }
}

// Head dim 64 (wav2vec2-base / -large): 53 KB of LDS at T = 199 without the V^T buffer => three workgroups per CU instead of two.
template <int NT>
__global__ __launch_bounds__(256, 2) void attention_tr_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                              int T, int H, float scale) {
    constexpr int D = 64, NKEY = NT * 16;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[NKEY * D];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[NKEY * D];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * D;
    stage_dma<NKEY, 256, 1>((char*)Ks, (char*)Vs, base, 0, ld, H, T, tid);
    __syncthreads();
    const read_v_tr<NT> read_v{(const __attribute__((address_space(3))) char*)LDS_PTR(Vs), lane};
    for (int qt = wv; qt * 16 < T; qt += 4)
        attend_tile<NT, D, 1>(base, 0, ld, Ks, read_v, ctx + (long)b * T * H + head * D, 0, H, T, D, scale, qt, fr, g);
}

// Dynamic LDS of the split kernels: both planes of K [keys][D] and V^T [D][keys + 64] (attention_x3_kernel: all nt * 16 keys;
// attention_x3_stream_kernel: one block of them), or of K and V row-major at head dim 64 (attention_x3_tr_kernel).
constexpr size_t att_x3_lds(int nt, int D) { return (size_t)2 * (nt * 16 * D + D * (nt * 16 + 64)) * 2; }
constexpr size_t att_x3_tr_lds(int nt) { return (size_t)4 * nt * 16 * 64 * 2; }

// fp32-class instance: q, k, v and the context are plane pairs in the split format of device_math.h; the softmax is fp32 as before
// and the probabilities are split before O^T = V^T P^T.  K and V^T (hi and lo) of one (clip, head) stay in LDS: 144 KB at T <= 256,
// head dim <= 64 => one workgroup per CU (attention is 4 % of the FLOPs); eight wavefronts share it, so the 13 query tiles of a
// 4 s clip take two rounds and each SIMD has a second wavefront to issue while the first waits on LDS.
template <int NT, int D>
__global__ __launch_bounds__(512, 1) void attention_x3_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                              long ctx_lo, int T, int H, int dm, float scale) {
    constexpr int NKEY = NT * 16, VP = NKEY + 64;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2][NKEY * D]
    _Float16* Vt = att_lds + 2 * NKEY * D;       // [2][D * VP]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    for (int pl = 0; pl < 2; ++pl)               // plane by plane: half the staging registers
        stage_regs<NKEY, D, 512, 2>(Ks + pl * NKEY * D, Vt + pl * D * VP, base + (pl ? qkv_lo : 0) + H, H, false, ld, dm / 8, T, 0, tid);
    __syncthreads();
    const read_v_t<NT, D> read_v{Vt, fr, g};
    for (int qt = wv; qt * 16 < T; qt += 8)      // 8 wavefronts (2 per SIMD): 13 query tiles at T = 199 take 2 rounds
        attend_tile<NT, D, 2>(base, qkv_lo, ld, Ks, read_v, ctx + (long)b * T * H + head * dm, ctx_lo, H, T, dm, scale, qt, fr, g);
}

// fp32-class attention for head dims 72 .. 128 (XLS-R-2B, the reference's own embedder: 1920 / 16 heads = 120): K and V^T of a
// whole clip in both planes do not fit 160 KB at D = 128, so the keys stream through LDS in blocks of NTB * 16 with an online
// softmax (running row maximum m and sum l in the log2 domain; O rescaled by 2^(m_old - m_new) when a block raises the
// maximum).  Eight wavefronts = eight query tiles per round; a 4 s clip (13 tiles) takes two rounds, each re-staging the
// blocks (the price of keeping one query tile's state per wavefront: 64 accumulator registers for O at D = 128).
template <int NTB, int D>
__global__ __launch_bounds__(512, 1) void attention_x3_stream_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                     long ctx_lo, int T, int H, int dm, float scale) {
    constexpr int KB = NTB * 16, VP = KB + 64, NS = (NTB + 1) / 2, KK = D / 32, DT = D / 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2][KB * D]
    _Float16* Vt = att_lds + 2 * KB * D;         // [2][D * VP]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * dm;
    const int nqt = (T + 15) / 16, nblk = (T + KB - 1) / KB;
    const read_v_t<NTB, D> read_v{Vt, fr, g};

    for (int q0 = 0; q0 < nqt; q0 += 8) {
        const int qt = q0 + wv;
        const bool live = qt < nqt;                  // wave-uniform; idle wavefronts still take part in staging and barriers
        const int qrow = qt * 16 + fr;
        const int qr = qrow < T ? qrow : T - 1;
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
                                          isv, ld, dm / 8, T, k0, tid);
            }
            __syncthreads();
            if (!live) continue;
            f32x4 s[NTB];
            score_tiles<NTB, D, 2>(s, Ks, q, fr, g);
            const float mx = mask_scale_max<NTB>(s, scale, k0, T, g);
            const float m_new = fmaxf(m_run, mx);     // finite: every block holds at least one key < T
            const float alpha = exp2f(m_run - m_new); // 0 for the first block (m_run = -inf)
            l_run = l_run * alpha + exp_sum<NTB, false>(s, m_new);
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[dt][0][r] *= alpha; o[dt][1][r] *= alpha; }
            // un-normalised probabilities (<= 1) as the split B operand, built per 32-key step right before its MFMAs (building all
            // NS pairs up front kept 32 more registers live and spilled 216 B per lane at D = 128: profiles/r03_xlsr2b_kernel_summary.txt);
            // the 1 / l normalisation happens once at the end
#pragma unroll
            for (int ss = 0; ss < NS; ++ss) {
                f16x8 p[2];
                pack_p<NTB, 2, false>(p, s, ss, 1.f);
                pv_step<DT, 2>(o, p, ss, read_v);
            }
        }
        if (live && qrow < T) store_ctx<DT, 2, true>(ctx + (long)b * T * H + head * dm, ctx_lo, (long)qrow * H, o, g, dm, 1.f / l_run);
    }
}

// fp32-class attention, head dim 64 (wav2vec2-base / -large): the split-format counterpart of attention_tr_kernel
// (attention_x3_kernel spent 35 % of its LDS cycles on bank conflicts of the transposing stores).  106 KB of LDS at T = 199.
template <int NT>
__global__ __launch_bounds__(512, 1) void attention_x3_tr_kernel(const _Float16* __restrict__ qkv, long qkv_lo, _Float16* __restrict__ ctx,
                                                                 long ctx_lo, int T, int H, float scale) {
    constexpr int D = 64, NKEY = NT * 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 att_lds[];
    _Float16* Ks = att_lds;                      // [2 planes][NKEY][64]
    _Float16* Vs = att_lds + 2 * NKEY * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * T * ld + head * D;
    stage_dma<NKEY, 512, 2>((char*)Ks, (char*)Vs, base, qkv_lo, ld, H, T, tid);
    __syncthreads();
    const read_v_tr<NT> read_v{(const __attribute__((address_space(3))) char*)LDS_PTR(Vs), lane};
    for (int qt = wv; qt * 16 < T; qt += 8)
        attend_tile<NT, D, 2>(base, qkv_lo, ld, Ks, read_v, ctx + (long)b * T * H + head * D, ctx_lo, H, T, D, scale, qt, fr, g);
}

}  // namespace advh

using namespace advh;

// f(NT) with the tile-count class NT (an integral_constant) of nt = ceil(T / 16) <= 16 key tiles
template <class F>
static void with_tile_class(int nt, F&& f) {
    if (nt <= 4) f(std::integral_constant<int, 4>{});
    else if (nt <= 8) f(std::integral_constant<int, 8>{});
    else if (nt <= 13) f(std::integral_constant<int, 13>{});
    else f(std::integral_constant<int, 16>{});
}

extern "C" int advh_attention_f16(const void* qkv, void* ctx, int B, int T, int H, int heads, advh_stream_t stream) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const float scale = 1.f / sqrtf((float)dm);
    const dim3 grid(heads, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    with_tile_class((T + 15) / 16, [&](auto cls) {
        constexpr int NT = decltype(cls)::value;
        if (dm == 64) hipLaunchKernelGGL((attention_tr_kernel<NT>), grid, block, 0, s, q, c, T, H, scale);   // DMA staging + transposing V^T reads
        else if (dm <= 32) hipLaunchKernelGGL((attention_kernel<NT, 32>), grid, block, 0, s, q, c, T, H, dm, scale);
        else if (dm <= 64) hipLaunchKernelGGL((attention_kernel<NT, 64>), grid, block, 0, s, q, c, T, H, dm, scale);
        else hipLaunchKernelGGL((attention_kernel<(NT == 8 ? 13 : NT), 128>), grid, block, 0, s, q, c, T, H, dm, scale);   // no 8 class at D = 128
    });
    return ADVH_LAUNCH_CHECK();
}

// Raise the dynamic-LDS limit of the split attention instances (advh_init).
int advh_init_attention() {
#define RAISE(kernel, bytes)                                                                                                        \
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) != hipSuccess) return ADVH_ELAUNCH;
#define X3(NT_) RAISE((attention_x3_kernel<NT_, 32>), att_x3_lds(NT_, 32)) RAISE((attention_x3_kernel<NT_, 64>), att_x3_lds(NT_, 64)) \
                RAISE(attention_x3_tr_kernel<NT_>, att_x3_tr_lds(NT_))
    X3(4) X3(8) X3(13) X3(16)
    RAISE((attention_x3_stream_kernel<7, 128>), att_x3_lds(7, 128))
#undef X3
#undef RAISE
    return ADVH_OK;
}

extern "C" int advh_attention_split(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, int B, int T, int H, int heads,
                                    advh_stream_t stream) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || heads <= 0 || H % heads || qkv_lo <= 0 || ctx_lo <= 0 || qkv_lo % 8 || ctx_lo % 4) return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const float scale = 1.f / sqrtf((float)dm);
    const dim3 grid(heads, B), block(512);
    hipStream_t s = (hipStream_t)stream;
    const _Float16* q = (const _Float16*)qkv;
    _Float16* c = (_Float16*)ctx;
    const long ql = (long)qkv_lo, cl = (long)ctx_lo;
    if (dm > 64)                                         // keys streamed in blocks of 112 with an online softmax
        hipLaunchKernelGGL((attention_x3_stream_kernel<7, 128>), grid, block, att_x3_lds(7, 128), s, q, ql, c, cl, T, H, dm, scale);
    else with_tile_class((T + 15) / 16, [&](auto cls) {
        constexpr int NT = decltype(cls)::value;
        if (dm == 64) hipLaunchKernelGGL((attention_x3_tr_kernel<NT>), grid, block, att_x3_tr_lds(NT), s, q, ql, c, cl, T, H, scale);
        else if (dm <= 32) hipLaunchKernelGGL((attention_x3_kernel<NT, 32>), grid, block, att_x3_lds(NT, 32), s, q, ql, c, cl, T, H, dm, scale);
        else hipLaunchKernelGGL((attention_x3_kernel<NT, 64>), grid, block, att_x3_lds(NT, 64), s, q, ql, c, cl, T, H, dm, scale);
    });
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention)
