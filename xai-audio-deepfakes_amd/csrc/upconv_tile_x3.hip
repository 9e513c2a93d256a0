// fp32-class line tile for the LAST decoder stage of the U-Net: up1 = ConvTranspose2d(64, 32, (2,1), stride (2,1)) folded into
// d1.block.0 = Conv2d(33, 32, 3, padding 1) + BatchNorm + LeakyReLU on split-format maps -- the split counterpart of
// upconv21_tile_kernel (upconv_tile.hip), built from it the way conv_taps2d_x3_kernel was built from conv_taps2d_kernel.
// Arithmetic of gemm_x3_kernel: per 32-deep k-block accx += Wh Xl; acc += Wh Xh; accx += Wl Xh, result acc + accx * 2^-11, then bias,
// LeakyReLU and the split store; K layout per row parity exactly gemm.plan_upconv2d's (zero-padded from 456 to 480 = 15 k-blocks):
//   k-blocks 0..11 : coarse tap t = s / 2 = 3 ti + tj, channels 32 (s & 1) .. + 31
//   k-blocks 12..14: fine taps 4 (s - 12) + g of the 8-channel (x, indicator, 0 ...) map, lane group g = one tap (taps 9..11: zero weights)
// so the outputs are bit-identical to the x3 implicit GEMM on the same maps.
// LDS plan (160 KiB per CU): both parities' weights in two planes are 2 x 60 KiB and do not fit next to any patch, so a workgroup owns
// ONE row parity: its composed weights stay resident (hi | lo, 60 KiB) and it walks tiles of 32 output rows x 16 columns, i.e. the 16
// rows of its parity: a 17 x 18 patch of the 64-channel coarse map and a 33 x 18 patch of the 8-channel map, both planes, in ONE
// buffer (98 KiB) -> 158 KiB, one workgroup of eight wavefronts per CU = two per SIMD.  Wavefront tile 32 channels x 32 positions
// (2 weight fragments x 2 position fragments): 8 KiB of fragments per 12 MFMAs.  The next tile's patch is requested after the last
// k-block's MFMAs and lands under the epilogue; the only wait is vmcnt(0) in front of the tile's barrier.  (Requesting the coarse part
// three k-blocks earlier, when its last fragments are read, measured the same: 712 / 727 against 711 / 724 us, so it is not done.)
// The two parities of a tile belong to workgroups blockIdx b and b ^ 8, which the dispatcher places on the same XCD (round robin over
// eight), so the second read of a coarse patch is served by that XCD's L2 rather than by HBM.
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

constexpr int UX_N = 32, UX_C0 = 64, UX_NS = 15, UX_NW = 8, UX_NTH = 64 * UX_NW;
constexpr int UX_WCH = UX_NS * UX_N * 4;                           // 16-byte chunks of one parity's weights per plane: 1 920
constexpr int UX_PR = 18, UX_CROWS = 17, UX_SROWS = 33;            // patch width; coarse / fine patch rows of one parity
constexpr int UX_PC = UX_CROWS * UX_PR, UX_PS = UX_SROWS * UX_PR;  // patch positions: 306 coarse, 594 fine
constexpr int UX_CCH = (UX_PC * 8 + 63) & ~63, UX_SCH = (UX_PS + 63) & ~63;   // chunks per plane (whole-wave loads): 2 496, 640
constexpr int UX_PLANE = (UX_CCH + UX_SCH) * 16;                   // one plane of the patch pair: 50 176 bytes
constexpr int UX_LDS = 2 * UX_WCH * 16 + 2 * UX_PLANE;             // 161 792
static_assert(UX_WCH % 64 == 0, "the weights are whole-wave loads");
static_assert(UX_LDS <= 160 * 1024, "one workgroup per CU");

__global__ __launch_bounds__(UX_NTH, 1)
void upconv21_tile_x3_kernel(const advh_upconv_desc p, long xc_lo, long xs_lo, long w_lo, long o_lo) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    char* Wl = lds;                                                // [hi | lo] x [15][32 rows (host-permuted)][32 k]
    char* Xl = lds + 2 * UX_WCH * 16;                              // [hi | lo] x [coarse 17 x 18 x 8 chunks | fine 33 x 18 chunks]
    const _Float16* Xc = (const _Float16*)p.Xc;
    const _Float16* Xs = (const _Float16*)p.Xs;
    const int Hf = 2 * p.Hc;
    const int Hpc = p.Hc + 2 * p.PHc, Wpc = p.W_ + 2 * p.PWc, Hps = Hf + 2 * p.PHs, Wps = p.W_ + 2 * p.PWs;
    const int Hpo = Hf + 2 * p.PHo, Wpo = p.W_ + 2 * p.PWo;
    const int tx = (p.W_ + 15) / 16, ty = (Hf + 31) / 32, ntiles = p.B * ty * tx;
    // workgroups b and b ^ 8 share a tile sequence (one parity each); the grid is a multiple of 16
    const int ph = (blockIdx.x >> 3) & 1, slot = (blockIdx.x & 7) + 8 * (blockIdx.x >> 4), nslots = gridDim.x >> 1;
    if (slot >= ntiles) return;
    auto origin = [&](int tile, int& b, int& y0, int& x0) {
        x0 = (tile % tx) * 16;
        const int r = tile / tx;
        y0 = (r % ty) * 32;
        b = r / ty;
    };
    // ---- this parity's weights: 64-byte LDS rows, chunk c of row r at slot c ^ ((r >> 1) & 2)
    const _Float16* Wg = (const _Float16*)p.W + (long)ph * (UX_WCH * 8);
    for (int i = tid; i < UX_WCH; i += UX_NTH) {
        const int row = i >> 2, pos = i & 3;
        const _Float16* src = Wg + (long)row * 32 + ((pos ^ ((row >> 1) & 2)) * 8);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(Wl + (size_t)(i - lane) * 16), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + w_lo), LDS_PTR(Wl + (size_t)UX_WCH * 16 + (size_t)(i - lane) * 16), 16, 0, 0);
    }
    auto load_patches = [&](int tile) {
        int b, y0, x0;
        origin(tile, b, y0, x0);
        char* ds = Xl + UX_CCH * 16;
        // coarse: rows y0 / 2 - 1 + ph .. + 16, columns x0 - 1 .. + 16 (clamped into the map: clamped rows only feed outputs that are
        // not written; filler chunks of the last wave load repeat row 0)
        for (int i = tid; i < UX_CCH; i += UX_NTH) {
            int row = i >> 3;
            const int pos = i & 7;
            if (row >= UX_PC) row = 0;
            const int gy = min((y0 >> 1) + p.PHc - 1 + ph + row / UX_PR, Hpc - 1), gx = min(x0 + p.PWc - 1 + row % UX_PR, Wpc - 1);
            const _Float16* src = Xc + (((long)b * Hpc + gy) * Wpc + gx) * UX_C0 + ((pos ^ ((i >> 3) & 7)) * 8);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(Xl + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + xc_lo), LDS_PTR(Xl + UX_PLANE + (size_t)(i - lane) * 16), 16, 0, 0);
        }
        // fine (8 channels = one chunk per pixel): rows y0 - 1 + ph .. + 32
        for (int i = tid; i < UX_SCH; i += UX_NTH) {
            const int row = i < UX_PS ? i : 0;
            const int gy = min(y0 + p.PHs - 1 + ph + row / UX_PR, Hps - 1), gx = min(x0 + p.PWs - 1 + row % UX_PR, Wps - 1);
            const _Float16* src = Xs + (((long)b * Hps + gy) * Wps + gx) * 8;
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(ds + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + xs_lo), LDS_PTR(ds + UX_PLANE + (size_t)(i - lane) * 16), 16, 0, 0);
        }
    };
    const int a0 = 2 * wv;                                         // this wavefront: output rows y = y0 + 2 (a0 + j) + ph, j = 0, 1
    float4 bias[2];                                                // channels 8 g + 4 e .. + 3
#pragma unroll
    for (int e = 0; e < 2; ++e) bias[e] = p.bias ? *(const float4*)(p.bias + g * 8 + e * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int wo0 = (fr * 4 + (g ^ ((fr >> 1) & 2))) * 16;         // fragment i: + i * 16 rows, k-block s: + s * 32 rows (64 bytes each)

    load_patches(slot);
    for (int tile = slot; tile < ntiles; tile += nslots) {
        f32x4 acc[2][2], accx[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; accx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        f16x8 fwh[2][2], fwl[2][2], fxh[2][2], fxl[2][2];
        auto fetch = [&](int set, int s) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int wo = wo0 + (s * UX_N + i * 16) * 64;
                fwh[set][i] = *(const f16x8*)(Wl + wo);
                fwl[set][i] = *(const f16x8*)(Wl + UX_WCH * 16 + wo);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int xo;
                if (s < 12) {
                    const int t = s >> 1, ti = t / 3, tj = t - ti * 3, c = (s & 1) * 4 + g;
                    const int row = (a0 + j + ti) * UX_PR + tj + fr;
                    xo = (row * 8 + (c ^ (row & 7))) * 16;
                } else {
                    const int tap = min(4 * (s - 12) + g, 8), kh = tap / 3, kw = tap - kh * 3;
                    xo = UX_CCH * 16 + ((2 * (a0 + j) + kh) * UX_PR + kw + fr) * 16;
                }
                fxh[set][j] = *(const f16x8*)(Xl + xo);
                fxl[set][j] = *(const f16x8*)(Xl + UX_PLANE + xo);
            }
        };
        auto mma = [&](int set) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxl[set][j], accx[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[set][i], fxh[set][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwl[set][i], fxh[set][j], accx[i][j], 0, 0, 0);
            }
        };
        // the patch, the previous epilogue's stores and (first tile) the weights must have landed: everything this thread requested
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        fetch(0, 0);
#pragma unroll
        for (int s = 0; s < UX_NS; ++s) {
            const int cur = s & 1;
            if (s + 1 < UX_NS) fetch(cur ^ 1, s + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(cur);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (tile + nslots < ntiles) {
            __syncthreads();                                       // every wavefront has read its last fragments of this patch
            load_patches(tile + nslots);
        }
        // ---- epilogue: join, bias, LeakyReLU, split stores of the interior positions
        int b, y0, x0;
        origin(tile, b, y0, x0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = y0 + 2 * (a0 + j) + ph, gx = x0 + fr;
            if (gy >= Hf || gx >= p.W_) continue;
            const long o = (((long)b * Hpo + gy + p.PHo) * Wpo + gx + p.PWo) * UX_N + g * 8;
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = fmaf(accx[0][j][r], SPLIT_LO_INV, acc[0][j][r]);
                v[4 + r] = fmaf(accx[1][j][r], SPLIT_LO_INV, acc[1][j][r]);
            }
            v[0] += bias[0].x; v[1] += bias[0].y; v[2] += bias[0].z; v[3] += bias[0].w;
            v[4] += bias[1].x; v[5] += bias[1].y; v[6] += bias[1].z; v[7] += bias[1].w;
            if (p.act == ADVH_ACT_LEAKY) {
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = v[r] > 0.f ? v[r] : p.slope * v[r];
            }
            store_h_rt<8>((_Float16*)p.out_h, o, o_lo, v);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace advh

using namespace advh;

extern "C" int advh_upconv21_tile_split_lds_bytes(void) { return UX_LDS; }

extern "C" int advh_upconv21_tile_split(const advh_upconv_desc* d, int Cc, int N, int64_t xc_lo, int64_t xs_lo, int64_t w_lo, int64_t o_lo,
                                        advh_stream_t stream) {
    if (!d || !d->Xc || !d->Xs || !d->W || !d->out_h || d->B <= 0 || d->Hc <= 0 || d->W_ <= 0) return ADVH_EINVAL;
    if (d->PHc < 1 || d->PWc < 1 || d->PHs < 1 || d->PWs < 1 || d->PHo < 0 || d->PWo < 0) return ADVH_EINVAL;
    if (Cc != UX_C0 || N != UX_N) return ADVH_EUNSUPPORTED;         // up1 + d1.block.0: 64 coarse channels, 32 outputs
    if (d->act != ADVH_ACT_NONE && d->act != ADVH_ACT_LEAKY) return ADVH_EINVAL;
    if (d->Xc == d->out_h || d->Xs == d->out_h) return ADVH_EINVAL;
    // the lo planes lie behind whole hi planes at 16-byte-aligned distances
    const long Hf = 2L * d->Hc;
    const long pc = (long)d->B * (d->Hc + 2 * d->PHc) * (d->W_ + 2 * d->PWc) * UX_C0, ps = (long)d->B * (Hf + 2 * d->PHs) * (d->W_ + 2 * d->PWs) * 8;
    const long po = (long)d->B * (Hf + 2 * d->PHo) * (d->W_ + 2 * d->PWo) * UX_N;
    if (xc_lo < pc || xs_lo < ps || o_lo < po || w_lo < 2L * UX_WCH * 8 || xc_lo % 8 || xs_lo % 8 || w_lo % 8 || o_lo % 8) return ADVH_EINVAL;
    const long ntiles = (long)d->B * ((Hf + 31) / 32) * ((d->W_ + 15) / 16);
    if (ntiles > 0x7fffffffL) return ADVH_EINVAL;
    if (advh_ensure_lds((const void*)upconv21_tile_x3_kernel) != ADVH_OK) return ADVH_ELAUNCH;
    const long grid = ntiles >= 128 ? 256 : 16 * ((ntiles + 7) / 8);      // pairs of workgroups (b, b ^ 8): a multiple of 16
    hipLaunchKernelGGL(upconv21_tile_x3_kernel, dim3((unsigned)grid), dim3(UX_NTH), UX_LDS, (hipStream_t)stream, *d, (long)xc_lo, (long)xs_lo,
                       (long)w_lo, (long)o_lo);
    return ADVH_LAUNCH_CHECK();
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_upconv_tile_x3)
