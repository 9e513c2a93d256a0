// fp32-class 2-D line tile: the 3x3 stride-1 "same" Conv2d layers of the U-Net's 32- and 64-channel ConvBlocks (addvisor.py:12-25,
// e1 / e2 / d2 / d1 .block.3) on split-format maps.  Geometry of conv_taps2d_kernel (conv_taps.hip): a workgroup owns 16 x 16 output
// positions and stages their 18 x 18 input patch ONCE (both planes, LDS DMA), so tap (kh, kw) of output (ly, lx) is patch row
// (ly + kh) * 18 + lx + kw -- 1.27 x over-read instead of the implicit GEMM's one input re-read per tap through the L2 -> LDS path.
// Arithmetic and K order of gemm_x3_kernel (as in conv_taps_x3_kernel): per 32-deep step accx += Wh Xl; acc += Wh Xh; accx += Wl Xh,
// steps tap-major (kh, kw) then input channel, result acc + accx * 2^-11, then bias and LeakyReLU: the outputs are bit-identical to the
// x3 implicit GEMM of gemm.plan_conv2d on the same maps.
// 32 channels: both planes of the 9-tap weights (36 KiB) stay resident; one patch buffer (42 KiB) -> 78 KiB, two workgroups of four
// wavefronts per CU.  Wavefront tile 32 channels x 64 positions (4 position fragments x 2 weight fragments).
// 64 channels: both planes are 144 KiB, so the weights stream tap by tap (16 KiB per tap) through a four-slot ring as in
// conv_taps_x3_kernel; one patch buffer (82 KiB) -> 146 KiB, one workgroup of eight wavefronts per CU.  Wavefront tile 64 channels x
// 32 positions (2 position fragments x 4 weight fragments).
// Either way two wavefronts per SIMD; 12 KiB of fragments per 24 MFMAs and wavefront.  The next tile's patch is requested after the
// last tap's MFMAs and lands under the epilogue.  Only interior positions are written: the destination's halo must already be zero.
// HEAD (32 channels, d1.block.3): the U-Net's 1x1 mask head + sigmoid (unet_head_kernel, unet_misc.hip) computed where the map is
// produced.  A lane's epilogue vector is one position's channels 8 g .. 8 g + 7, i.e. exactly one of the head kernel's four 8-channel
// fmaf chains; the chains of g = 0 .. 3 sit 16 lanes apart and meet in two xor-shuffles in the head kernel's order (s0 + s1) + (s2 + s3).
// The chain runs on hi + lo * 2^-11 of the planes that WOULD have been stored (same conversion, same range flag), so logits and mask
// are bit-identical to the two-kernel form; the 32-channel map itself is not written.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"

namespace advh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// LDS row swizzle and MFMA row -> output channel map of conv_taps.hip (same layouts, so the same conflict-free reads)
template <int C> __device__ __forceinline__ int swz2(int r) { return C == 64 ? (r & 7) : ((r >> 1) & 2); }
__device__ __forceinline__ int cout_of2(int R) { return ((R >> 5) << 5) + (((R >> 2) & 3) << 3) + (((R >> 4) & 1) << 2) + (R & 3); }

template <int C> struct Taps2dX3Cfg;
template <> struct Taps2dX3Cfg<32> { static constexpr int NJ = 4, NW = 4, NSLOT = 9; static constexpr bool RES = true; };
template <> struct Taps2dX3Cfg<64> { static constexpr int NJ = 2, NW = 8, NSLOT = 4; static constexpr bool RES = false; };

constexpr int T2_PR = 18, T2_SR = T2_PR * T2_PR;

template <int C> constexpr int taps2d_x3_src() { return (T2_SR * (C / 8) + 63) & ~63; }    // patch chunks per plane (whole wave loads)
// the optional 1x1 head of the 32-channel form: w [32] fp32, mask / logits fp32 [B][H][W] (logits may be null)
struct taps2d_head { const float* w; float bias; float* mask; float* logits; };

template <int C> constexpr int taps2d_x3_lds() { return Taps2dX3Cfg<C>::NSLOT * 2 * C * C * 2 + 2 * taps2d_x3_src<C>() * 16; }

template <int C, bool HEAD>
__global__ __launch_bounds__(64 * Taps2dX3Cfg<C>::NW, 2 * 4 / Taps2dX3Cfg<C>::NW)
void conv_taps2d_x3_kernel(const advh_taps2d_desc p, long x_lo, long w_lo, long o_lo, const taps2d_head hd) {
    static_assert(!HEAD || C == 32, "the mask head is a 32-channel dot product (unet_head_kernel's four 8-channel chains)");
    constexpr int NJ = Taps2dX3Cfg<C>::NJ, NW = Taps2dX3Cfg<C>::NW, NSLOT = Taps2dX3Cfg<C>::NSLOT;
    constexpr bool RES = Taps2dX3Cfg<C>::RES;
    static_assert(NJ * NW == 16, "one 16 x 16 output tile per workgroup");
    constexpr int CH = C / 8, CT = C / 16, KS = C / 32, NTH = 64 * NW, WTAP = C * C * 2, SRC = taps2d_x3_src<C>();
    constexpr int AHEAD = NSLOT - 1, WPT = RES ? 0 : 2 * (C * CH / NTH);   // WPT: DMA instructions per thread and streamed tap
    static_assert(RES || C * CH == NTH, "a streamed tap is one 16-byte chunk per thread and plane");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    char* Wl = lds;                                                // NSLOT slots x [hi | lo] x [C][C] halfs
    char* Xl = lds + NSLOT * 2 * WTAP;                             // [hi | lo] x [SRC chunks]: the 18 x 18 patch
    const _Float16* Wg = (const _Float16*)p.W;
    const _Float16* X = (const _Float16*)p.X;
    const int Hp = p.H + 2 * p.PH, Wp = p.W_ + 2 * p.PW;
    const int tx = (p.W_ + 15) / 16, ty = (p.H + 15) / 16, ntiles = p.B * ty * tx;
    auto origin = [&](int tile, int& b, int& y0, int& x0) {
        x0 = (tile % tx) * 16;
        const int r = tile / tx;
        y0 = (r % ty) * 16;
        b = r / ty;
    };
    auto load_weights = [&](int t, int slot) {
        char* dst = Wl + (size_t)slot * 2 * WTAP;
        for (int i = tid; i < C * CH; i += NTH) {                  // i = lds chunk index (wave-linear; C * CH is a multiple of 64)
            const int row = i / CH, pos = i % CH;
            const _Float16* src = Wg + ((long)t * C + cout_of2(row)) * C + ((pos ^ swz2<C>(row)) * 8);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(dst + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + w_lo), LDS_PTR(dst + WTAP + (size_t)(i - lane) * 16), 16, 0, 0);
        }
    };
    auto load_patch = [&](int tile) {
        int b, y0, x0;
        origin(tile, b, y0, x0);
        for (int i = tid; i < SRC; i += NTH) {
            int row = i / CH;
            const int pos = i % CH;
            if (row >= T2_SR) row = 0;                             // filler chunks of the last wave load: an unread slot
            // padded coordinates of patch row `row`, clamped into the map (clamped rows only feed outputs that are not written)
            const int gy = min(y0 + p.PH - 1 + row / T2_PR, Hp - 1), gx = min(x0 + p.PW - 1 + row % T2_PR, Wp - 1);
            const _Float16* src = X + (((long)b * Hp + gy) * Wp + gx) * C + ((pos ^ swz2<C>(i / CH)) * 8);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(Xl + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + x_lo), LDS_PTR(Xl + (size_t)SRC * 16 + (size_t)(i - lane) * 16), 16, 0, 0);
        }
    };
    float4 bias[CT];                                               // bias[2q + e] = channels 32 q + 8 g + 4 e .. + 3
#pragma unroll
    for (int i = 0; i < CT; ++i)
        bias[i] = p.bias ? *(const float4*)(p.bias + (i >> 1) * 32 + g * 8 + (i & 1) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    float hw[8];                                                   // HEAD: the head weights of this lane's channels 8 g .. 8 g + 7
#pragma unroll
    for (int r = 0; r < 8; ++r) hw[r] = HEAD ? hd.w[g * 8 + r] : 0.f;

    // streamed form: global tap counter n (tap n % 9 of the workgroup's n / 9-th tile) lives in slot n % NSLOT, taps 0 .. AHEAD-1 up front
    const int mytiles = (int)blockIdx.x < ntiles ? (ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int ntot = mytiles * 9;
    if (RES) {
        if (mytiles)
            for (int t = 0; t < 9; ++t) load_weights(t, t);
    } else {
        for (int n = 0; n < AHEAD && n < ntot; ++n) load_weights(n % 9, n % NSLOT);
    }
    if (mytiles) load_patch(blockIdx.x);
    int n = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        f32x4 acc[CT][NJ], accx[CT][NJ];
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        f16x8 fwh[2][CT], fwl[2][CT], fxh[2][NJ], fxl[2][NJ];
        // fragments of 32-deep step (tap t = kh * 3 + kw, ks) from weight slot `slot`; (16 i + fr) swizzles like fr
        auto fetch = [&](int set, int slot, int t, int ks) {
            const char* wb = Wl + (size_t)slot * 2 * WTAP;
            const int c = ks * 4 + g, kh = t / 3, kw = t - kh * 3;
#pragma unroll
            for (int i = 0; i < CT; ++i) {
                const int wo = ((i * 16 + fr) * CH + (c ^ swz2<C>(fr))) * 16;
                fwh[set][i] = *(const f16x8*)(wb + wo);
                fwl[set][i] = *(const f16x8*)(wb + WTAP + wo);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = (wv * NJ + j + kh) * T2_PR + kw + fr;
                const int xo = (row * CH + (c ^ swz2<C>(row))) * 16;
                fxh[set][j] = *(const f16x8*)(Xl + xo);
                fxl[set][j] = *(const f16x8*)(Xl + (size_t)SRC * 16 + xo);
            }
        };
        auto mma = [&](int set) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
#pragma unroll
                for (int i = 0; i < CT; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxl[set][j], accx[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < CT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxh[set][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < CT; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwl[set][i], fxh[set][j], accx[i][j], 0, 0, 0);
            }
        };
        auto slot_of = [&](int t) { return RES ? t : (n + t) % NSLOT; };   // n = this tile's tap 0
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t == 0 || !RES) {
                // t = 0: the patch, the previous epilogue's stores and (streamed) taps n, n + 1 must have landed -- everything; later taps:
                // all but the DMA instructions of the youngest requested tap (n + t + 2; at the workgroup's last taps, where none was
                // requested, everything).  The barrier then also means every wavefront is done with tap n + t - 1, whose ring slot the
                // request below reuses.
                if (t == 0 || n + t + 2 >= ntot) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WPT) : "memory");
                __syncthreads();
                if (!RES && n + t + AHEAD < ntot) load_weights((n + t + AHEAD) % 9, (n + t + AHEAD) % NSLOT);
            }
            if (t == 0) fetch(0, slot_of(0), 0, 0);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int s = t * KS + ks, cur = s & 1;
                if (ks + 1 < KS) fetch(cur ^ 1, slot_of(t), t, ks + 1);
                else if (t + 1 < 9) fetch(cur ^ 1, slot_of(t + 1), t + 1, 0);   // tap t + 1's weights: covered by this tap's barrier
                __builtin_amdgcn_sched_barrier(0);
                mma(cur);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        n += 9;
        if (tile + (int)gridDim.x < ntiles) {
            __syncthreads();                                       // every wavefront has read its last fragments of this patch
            load_patch(tile + gridDim.x);
        }
        // ---- epilogue: join, bias, LeakyReLU, split stores of the interior positions
        int b, y0, x0;
        origin(tile, b, y0, x0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int gy = y0 + wv * NJ + j, gx = x0 + fr;
            const bool inside = gy < p.H && gx < p.W_;
            if (!HEAD && !inside) continue;                        // HEAD: every lane stays for the shuffles
            const long pos = ((long)b * Hp + gy + p.PH) * Wp + gx + p.PW;
#pragma unroll
            for (int q = 0; q < CT / 2; ++q) {
                const long o = pos * C + q * 32 + g * 8;
                float v[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = fmaf(accx[2 * q][j][r], SPLIT_LO_INV, acc[2 * q][j][r]);
                    v[4 + r] = fmaf(accx[2 * q + 1][j][r], SPLIT_LO_INV, acc[2 * q + 1][j][r]);
                }
                v[0] += bias[2 * q].x; v[1] += bias[2 * q].y; v[2] += bias[2 * q].z; v[3] += bias[2 * q].w;
                v[4] += bias[2 * q + 1].x; v[5] += bias[2 * q + 1].y; v[6] += bias[2 * q + 1].z; v[7] += bias[2 * q + 1].w;
                if (p.act == ADVH_ACT_LEAKY) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] = v[r] > 0.f ? v[r] : p.slope * v[r];
                }
                if (!HEAD) {
                    store_h_rt<8>((_Float16*)p.out_h, o, o_lo, v);
                } else {
                    // unet_head_kernel on the value it would have loaded back: chain s_g of sequential fmaf from 0.f over channels
                    // 8 g .. 8 g + 7, (s0 + s1) + (s2 + s3), + bias, sigmoid.  Positions outside the map convert zeros (their
                    // accumulators hold clamped patch rows, which must not touch the range flag).
                    if (!inside) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) v[r] = 0.f;
                    }
                    f16x8 hv, lv;
                    split_f32_vec<8>(v, hv, lv);
                    float s = 0.f;
#pragma unroll
                    for (int r = 0; r < 8; ++r) s = fmaf(join_f32(hv[r], lv[r]), hw[r], s);
                    s += __shfl_xor(s, 16, 64);
                    s += __shfl_xor(s, 32, 64);
                    s += hd.bias;
                    if (g == 0 && inside) {
                        const long i = ((long)b * p.H + gy) * p.W_ + gx;
                        if (hd.logits) hd.logits[i] = s;
                        hd.mask[i] = 1.f / (1.f + expf(-s));
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace advh

// Argument check shared by the two entry points (conv_taps2d_x3.hip: the plain layer, out_h written; conv_taps2d_head_x3.hip: the
// 32-channel layer with the mask head, hd != nullptr).  ADVH_OK and the persistent grid, or the error to return.
inline int advh_taps2d_split_check(const advh_taps2d_desc* d, int C, int64_t x_lo, int64_t w_lo, int64_t o_lo, const advh::taps2d_head* hd,
                                   int lds, long* grid) {
    if (!d || !d->X || !d->W || (!hd && !d->out_h) || d->B <= 0 || d->H <= 0 || d->W_ <= 0 || d->PH < 1 || d->PW < 1) return ADVH_EINVAL;
    if (hd && (!hd->w || !hd->mask)) return ADVH_EINVAL;
    if (C != 32 && (hd || C != 64)) return ADVH_EUNSUPPORTED;
    if (d->act != ADVH_ACT_NONE && d->act != ADVH_ACT_LEAKY) return ADVH_EINVAL;
    if (!hd && d->X == d->out_h) return ADVH_EINVAL;              // other workgroups still read the patch rows a tile overwrites
    // the lo planes lie behind whole hi planes (they never overlap them) at 16-byte-aligned distances
    const long plane = (long)d->B * (d->H + 2 * d->PH) * (d->W_ + 2 * d->PW) * C;
    if (x_lo < plane || (!hd && o_lo < plane) || w_lo < 9L * C * C || x_lo % 8 || w_lo % 8 || (!hd && o_lo % 8)) return ADVH_EINVAL;
    const long ntiles = (long)d->B * ((d->H + 15) / 16) * ((d->W_ + 15) / 16);
    if (ntiles > 0x7fffffffL) return ADVH_EINVAL;
    const long per_cu = 160 * 1024 / lds;                          // 32 channels: two workgroups per CU, 64 channels: one
    *grid = ntiles < 256 * per_cu ? ntiles : 256 * per_cu;
    return ADVH_OK;
}
