// fp32-class line tile for e2.block.0 of the U-Net: Conv2d(32, 64, (5, 3), stride (2, 1), padding (2, 1)) + folded BatchNorm +
// LeakyReLU (addvisor.py:32) on split-format maps -- the split counterpart of conv53s21_tile_kernel (conv_s21_tile.hip), built the
// way conv_taps2d_x3_kernel<64> was built from conv_taps2d_kernel: that kernel's geometry idea (a staged input patch, tap = a patch
// offset) with the arithmetic and K order of gemm_x3_kernel.  Per 32-deep step accx += Wh Xl; acc += Wh Xh; accx += Wl Xh, steps =
// taps kh * 3 + kw of gemm.plan_conv2d (K = 15 x 32 = 480, zero-padded to 512: the sixteenth step multiplies zero weights with tap 0's
// patch data, as the GEMM's ktab filler does), result acc + accx * 2^-11, then bias, LeakyReLU and the split store: the outputs are
// bit-identical to the x3 implicit GEMM on the same maps.
// LDS plan (160 KiB per CU): both weight planes are 64 x 512 x 2 x 2 B = 128 KiB and leave room for a 4 x 16 tile only (6 fragment
// reads per 6 MFMAs and wavefront), so the weights stream instead: a ring unit is one 64-deep k-block of the GEMM (two taps, 64 rows x
// 64 k x 2 planes = 16 KiB), four slots, unit n + 3 requested when unit n starts, counted vmcnt -- conv_taps2d_x3_kernel<64>'s ring with
// 8 units per tile in place of 9.  That frees the space for a 16 x 16 output tile: its 35 x 18 patch of the 32-channel input (row pitch 20),
// both planes, is 88 KiB -> 152 KiB, one workgroup of eight wavefronts per CU = two per SIMD.  Wavefront tile 64 channels x 32 positions
// (4 weight fragments x 2 position fragments): 12 KiB of fragments per 24 MFMAs.  Per tile 216 KiB of fill against 3 072 MFMAs.
// The next tile's patch is requested after the last k-block's MFMAs and lands under the epilogue.
// Only interior positions are written: the destination's halo must already be zero.
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

constexpr int SX_CI = 32, SX_CO = 64, SX_KW = 3, SX_NT = 15, SX_NKB = 8;          // 15 taps in 8 k-blocks of two 32-deep steps
constexpr int SX_NW = 8, SX_NTH = 64 * SX_NW, SX_NJ = 2, SX_NSLOT = 4, SX_AHEAD = SX_NSLOT - 1;
// patch 35 x 18 positions at a row pitch of 20: a pitch of 4 (mod 8) makes the swizzle bit of patch row 2 Y + kh, column kw + fr a
// function of (kh & 1, kw, fr) alone, so a wavefront's 30 fragment addresses per step pair are six registers plus immediate offsets
constexpr int SX_PR = 20, SX_PCOLS = 18, SX_PROWS = 2 * 15 + 5, SX_POS = SX_PROWS * SX_PR;
constexpr int SX_CH = SX_CI / 8;                                                    // 16-byte chunks per patch position
constexpr int SX_SRC = (SX_POS * SX_CH + 63) & ~63;                                 // patch chunks per plane (whole-wave loads): 2 816
constexpr int SX_WKB = SX_CO * 64 * 2;                                              // one plane of a k-block: 8 KiB
constexpr int SX_WPT = 2 * (SX_CO * 8 / SX_NTH);                                    // DMA instructions per thread and k-block
constexpr int SX_BIAS = SX_NSLOT * 2 * SX_WKB + 2 * SX_SRC * 16;                    // the 64 bias values sit behind the patch
constexpr int SX_LDS = SX_BIAS + SX_CO * 4;                                         // 155 904
static_assert(SX_CO * 8 == SX_NTH, "a k-block is one 16-byte chunk per thread and plane");
static_assert(SX_NKB % SX_NSLOT == 0, "a k-block keeps its ring slot from tile to tile");
static_assert(SX_LDS <= 160 * 1024, "one workgroup per CU");

__global__ __launch_bounds__(SX_NTH, 1)
void conv53s21_tile_x3_kernel(const advh_convs21_desc p, long x_lo, long w_lo, long o_lo) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    char* Wl = lds;                                                // SX_NSLOT slots x [hi | lo] x [64 rows (host-permuted)][64 k]
    char* Xl = lds + SX_NSLOT * 2 * SX_WKB;                        // [hi | lo] x [SX_SRC chunks]: the 35 x 18 patch
    const _Float16* Wg = (const _Float16*)p.W;
    const _Float16* X = (const _Float16*)p.X;
    const int Hi = 2 * p.Ho;
    const int Hpi = Hi + 2 * p.PHi, Wpi = p.W_ + 2 * p.PWi, Hpo = p.Ho + 2 * p.PHo, Wpo = p.W_ + 2 * p.PWo;
    const int tx = (p.W_ + 15) / 16, ty = (p.Ho + 15) / 16, ntiles = p.B * ty * tx;
    auto origin = [&](int tile, int& b, int& y0, int& x0) {
        x0 = (tile % tx) * 16;
        const int r = tile / tx;
        y0 = (r % ty) * 16;
        b = r / ty;
    };
    // k-block kb: 128-byte LDS rows, chunk c of row r at slot c ^ (r & 7)
    auto load_weights = [&](int kb, int slot) {
        char* dst = Wl + (size_t)slot * 2 * SX_WKB;
        const int row = tid >> 3, pos = tid & 7;
        const _Float16* src = Wg + ((long)kb * SX_CO + row) * 64 + ((pos ^ (row & 7)) * 8);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(dst + (size_t)(tid - lane) * 16), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + w_lo), LDS_PTR(dst + SX_WKB + (size_t)(tid - lane) * 16), 16, 0, 0);
    };
    auto load_patch = [&](int tile) {
        int b, y0, x0;
        origin(tile, b, y0, x0);
        for (int i = tid; i < SX_SRC; i += SX_NTH) {
            int row = i / SX_CH;
            const int pos = i % SX_CH;
            if (row >= SX_POS) row = 0;                            // filler chunks of the last wave load: an unread slot
            // patch row 0 = input row 2 y0 - 2, column 0 = x0 - 1 (padded coordinates, clamped into the map: clamped positions only
            // feed outputs that are not written)
            const int gy = min(2 * y0 + p.PHi - 2 + row / SX_PR, Hpi - 1), gx = min(x0 + p.PWi - 1 + min(row % SX_PR, SX_PCOLS - 1), Wpi - 1);
            const _Float16* src = X + (((long)b * Hpi + gy) * Wpi + gx) * SX_CI + ((pos ^ (((i / SX_CH) >> 1) & 2)) * 8);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(Xl + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + x_lo), LDS_PTR(Xl + (size_t)SX_SRC * 16 + (size_t)(i - lane) * 16), 16, 0, 0);
        }
    };
    // the bias waits in LDS for the epilogue (16 registers that the K loop has no room for); visible after the first tile's barrier
    const float* Bl = (const float*)(lds + SX_BIAS);
    if (tid < SX_CO) ((float*)(lds + SX_BIAS))[tid] = p.bias ? p.bias[tid] : 0.f;

    // global k-block counter n (k-block n % 8 of the workgroup's n / 8-th tile) lives in slot n % SX_NSLOT = (n % 8) % SX_NSLOT: a k-block
    // has the same slot in every tile, so the fragment addresses are compile-time offsets.  The first SX_AHEAD k-blocks up front
    const int mytiles = (int)blockIdx.x < ntiles ? (ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int ntot = mytiles * SX_NKB;
    for (int n = 0; n < SX_AHEAD && n < ntot; ++n) load_weights(n % SX_NKB, n % SX_NSLOT);
    if (mytiles) load_patch(blockIdx.x);
    int n = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        f32x4 acc[4][SX_NJ], accx[4][SX_NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < SX_NJ; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        f16x8 fwh[2][4], fwl[2][4], fxh[2][SX_NJ], fxl[2][SX_NJ];
        // patch position (2 Y + kh) * 20 + kw + fr: bit 2 of it, which selects the swizzle, is (kh & 1) ^ bit 2 of (kw + fr)
        auto xbase = [&](int khp, int kw) {
            const int x = kw + fr;
            return ((wv * SX_NJ * 2 * SX_PR + x) * SX_CH + (g ^ (2 * (khp ^ ((x >> 2) & 1))))) * 16;
        };
        // fragments of 32-deep step s (tap s = kh * 3 + kw; step 15 = the zero-weight padding on tap 0's data) from weight slot `slot`
        auto fetch = [&](int set, int slot, int s) {
            const char* wb = Wl + (size_t)slot * 2 * SX_WKB;
            const int c = (s & 1) * 4 + g, t = s < SX_NT ? s : 0, kh = t / SX_KW, kw = t - kh * SX_KW;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int wo = ((i * 16 + fr) * 8 + (c ^ (fr & 7))) * 16;
                fwh[set][i] = *(const f16x8*)(wb + wo);
                fwl[set][i] = *(const f16x8*)(wb + SX_WKB + wo);
            }
#pragma unroll
            for (int j = 0; j < SX_NJ; ++j) {
                const int xo = xbase(kh & 1, kw) + (2 * j + kh) * SX_PR * SX_CH * 16;
                fxh[set][j] = *(const f16x8*)(Xl + xo);
                fxl[set][j] = *(const f16x8*)(Xl + (size_t)SX_SRC * 16 + xo);
            }
        };
        auto mma = [&](int set) {
#pragma unroll
            for (int j = 0; j < SX_NJ; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxl[set][j], accx[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxh[set][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwl[set][i], fxh[set][j], accx[i][j], 0, 0, 0);
            }
        };
#pragma unroll
        for (int kb = 0; kb < SX_NKB; ++kb) {
            // kb = 0: the patch, the previous epilogue's stores and k-blocks n, n + 1 must have landed -- everything; later k-blocks: all
            // but the DMA instructions of the youngest requested one (n + kb + 2; at the workgroup's last k-blocks, where none was
            // requested, everything).  The barrier then also means every wavefront is done with k-block n + kb - 1, whose ring slot the
            // request below reuses.
            if (kb == 0 || n + kb + 2 >= ntot) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SX_WPT) : "memory");
            __syncthreads();
            if (n + kb + SX_AHEAD < ntot) load_weights((kb + SX_AHEAD) % SX_NKB, (kb + SX_AHEAD) % SX_NSLOT);
            if (kb == 0) fetch(0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int s = kb * 2 + ks, cur = s & 1;
                if (ks == 0) fetch(cur ^ 1, kb % SX_NSLOT, s + 1);
                else if (kb + 1 < SX_NKB) fetch(cur ^ 1, (kb + 1) % SX_NSLOT, s + 1);   // k-block kb + 1: covered by this k-block's barrier
                __builtin_amdgcn_sched_barrier(0);
                mma(cur);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        n += SX_NKB;
        if (tile + (int)gridDim.x < ntiles) {
            __syncthreads();                                       // every wavefront has read its last fragments of this patch
            load_patch(tile + gridDim.x);
        }
        // ---- epilogue: join, bias, LeakyReLU, split stores of the interior positions
        int b, y0, x0;
        origin(tile, b, y0, x0);
        float4 bias[4];                                            // bias[2q + e] = channels 32 q + 8 g + 4 e .. + 3
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[i] = *(const float4*)(Bl + (i >> 1) * 32 + g * 8 + (i & 1) * 4);
#pragma unroll
        for (int j = 0; j < SX_NJ; ++j) {
            const int gy = y0 + wv * SX_NJ + j, gx = x0 + fr;
            if (gy >= p.Ho || gx >= p.W_) continue;
            const long pos = ((long)b * Hpo + gy + p.PHo) * Wpo + gx + p.PWo;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const long o = pos * SX_CO + q * 32 + g * 8;
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
                store_h_rt<8>((_Float16*)p.out_h, o, o_lo, v);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace advh

using namespace advh;

extern "C" int advh_conv53s21_tile_split_lds_bytes(void) { return SX_LDS; }

extern "C" int advh_conv53s21_tile_split(const advh_convs21_desc* d, int Ci, int N, int64_t x_lo, int64_t w_lo, int64_t o_lo, advh_stream_t stream) {
    if (!d || !d->X || !d->W || !d->out_h || d->B <= 0 || d->Ho <= 0 || d->W_ <= 0) return ADVH_EINVAL;
    if (d->PHi < 2 || d->PWi < 1 || d->PHo < 0 || d->PWo < 0) return ADVH_EINVAL;
    if (Ci != SX_CI || N != SX_CO) return ADVH_EUNSUPPORTED;        // e2.block.0: 32 input channels, 64 outputs
    if (d->act != ADVH_ACT_NONE && d->act != ADVH_ACT_LEAKY) return ADVH_EINVAL;
    if (d->X == d->out_h) return ADVH_EINVAL;
    // the lo planes lie behind whole hi planes at 16-byte-aligned distances
    const long px = (long)d->B * (2L * d->Ho + 2 * d->PHi) * (d->W_ + 2 * d->PWi) * SX_CI;
    const long po = (long)d->B * (d->Ho + 2 * d->PHo) * (d->W_ + 2 * d->PWo) * SX_CO;
    if (x_lo < px || o_lo < po || w_lo < (long)SX_NKB * SX_CO * 64 || x_lo % 8 || w_lo % 8 || o_lo % 8) return ADVH_EINVAL;
    const long ntiles = (long)d->B * ((d->Ho + 15) / 16) * ((d->W_ + 15) / 16);
    if (ntiles > 0x7fffffffL) return ADVH_EINVAL;
    if (advh_ensure_lds((const void*)conv53s21_tile_x3_kernel) != ADVH_OK) return ADVH_ELAUNCH;
    const long grid = ntiles < 256 ? ntiles : 256;
    hipLaunchKernelGGL(conv53s21_tile_x3_kernel, dim3((unsigned)grid), dim3(SX_NTH), SX_LDS, (hipStream_t)stream, *d, (long)x_lo, (long)w_lo,
                       (long)o_lo);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_conv_s21_tile_x3)
