// Ragged STFT and masked ISTFT for gfx950: clip b of a [B][L] buffer is transformed as its first lens[b] samples run alone.
//
// advh_stft_forward_ragged is advh_stft_forward's plain forward (stft.hip, stft_fwd_kernel<FB, 0>) and
// advh_istft_masked_c64_ragged the complex masked inverse (istft_kernel<3, FB>), both with every bound of a clip taken from
// L_b = clamp(lens[b], 513, L), T_b = 1 + L_b / hop: the reflection happens at L_b, frames >= T_b and samples >= L_b are
// written as zeros and nothing past the clip's extent is read.  The arithmetic per frame and per sample is the sibling's,
// statement for statement, so a clip's results equal the sibling's on the cropped clip bit for bit.
//
// The kernels of stft.hip take their arguments by value in a fixed order that its recorded device assembly depends on, so the
// per-clip bound could not be added there: this file carries its own narrowed copies of the wavefront transform, the LDS
// carve and the mask factor, and its own twiddle table (filled by advh_init through advh_init_stft_ragged).
#include <hip/hip_runtime.h>
#include "addvisor_hip.h"
#include "common.h"
#include "fft512.h"

namespace advh {
namespace stft_ragged {

__device__ cf g_twiddle[1024];   // e^{+2 pi i k / 1024}
static bool g_init_done[64] = {false};
static bool init_done_here() { int dev = 0; return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && g_init_done[dev]; }

constexpr int NFFT = 1024;
constexpr int NBIN = 513;
constexpr int THREADS = 512;           // 8 wavefronts, as in stft.hip

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct LaneTw { cf p8[7], p64[7], glue[4]; };
__device__ __forceinline__ void load_lane_twiddles(int lane, LaneTw& t) {
    fft512_lane_twiddles<8>(g_twiddle, lane, t.p8);
    fft512_lane_twiddles<64>(g_twiddle, lane, t.p64);
#pragma unroll
    for (int q = 0; q < 4; ++q) t.glue[q] = g_twiddle[lane + 1 + 64 * q];
}

// forward: inputs in registers (FROM_REGS); inverse: outputs stay in registers (TO_REGS) -- the two forms stft.hip runs
template <int DIR, bool FROM_REGS, bool TO_REGS>
__device__ __forceinline__ void fft512_wave(float* re, float* im, int lane, const LaneTw& t, cf (&v)[8]) {
    if (FROM_REGS) dft8<DIR>(v);
    else { fft512_pass_load_tw<DIR, 1>(re, im, lane, t.p8, v); wave_fence(); }
    fft512_pass_store<1>(re, im, lane, v);
    wave_fence();
    fft512_pass_load_tw<DIR, 8>(re, im, lane, t.p8, v);
    wave_fence();
    fft512_pass_store<8>(re, im, lane, v);
    wave_fence();
    fft512_pass_load_tw<DIR, 64>(re, im, lane, t.p64, v);
    if (!TO_REGS) {
        wave_fence();
        fft512_pass_store<64>(re, im, lane, v);
        wave_fence();
    }
}

// row pitch of the LDS tile: conflict-free transposed walk (stft.hip, RowPitch)
template <int FB> struct RowPitch { static constexpr int value = FFT_ROW + ((32 / FB - FFT_ROW % 32) + 32) % 32; };
static_assert(RowPitch<8>::value % 32 == 4 && RowPitch<16>::value % 32 == 2, "row pitch");

__device__ __forceinline__ float mask_factor(float m, float M, int mode) {
    if (mode == ADVH_MASK_LINEAR) return m;
    if (M < 1e-12f) return m;
    return (__builtin_amdgcn_exp2f(m * __builtin_amdgcn_logf(1.f + M)) - 1.f) * __builtin_amdgcn_rcpf(M);
}

// The clip's own sample count: no content of `lens` moves an access out of the clip's row.
__device__ __forceinline__ int clip_samples(const int* __restrict__ lens, int b, int L) {
    const int n = lens[b];
    return n < NFFT / 2 + 1 ? NFFT / 2 + 1 : n > L ? L : n;
}

// ------------------------------------------------------------------------------------------ forward
template <int FB>
__global__ __launch_bounds__(THREADS, 6) void stft_fwd_ragged_kernel(
    const float* __restrict__ wave, long wave_stride, const int* __restrict__ lens, int L, int hop, int win,
    const float* __restrict__ window, float* __restrict__ X, float* __restrict__ mag, float* __restrict__ phase, int T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWP = RowPitch<FB>::value;
    float* re = smem;
    float* im = smem + FB * ROWP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, tA = blockIdx.x * FB;
    const int left = (NFFT - win) / 2;
    const int Lb = clip_samples(lens, b, L);
    const int Tb = 1 + Lb / hop;                      // <= T
    const int nvalid = min(FB, T - tA);               // frames of the buffer this workgroup owns

    if (tA >= Tb) {                                   // past the clip: zeros in every requested output (workgroup-uniform)
        for (int idx = tid; idx < NBIN * FB; idx += THREADS) {
            const int tl = idx & (FB - 1), k = idx / FB;
            if (tl >= nvalid) continue;
            const long o = ((long)b * NBIN + k) * T + tA + tl;
            if (X) reinterpret_cast<float2*>(X)[o] = make_float2(0.f, 0.f);
            if (mag) mag[o] = 0.f;
            if (phase) phase[o] = 0.f;
        }
        return;
    }

    // one wavefront per frame: z[n] = x[2n] + i x[2n+1] straight from global memory, FFT512, real-transform glue
    const float* w = wave + (long)b * wave_stride;
#pragma unroll 1
    for (int f = wv; f < FB; f += THREADS / 64) {
        if (tA + f >= Tb) break;                      // wave-uniform
        // the lane index, opaque per iteration (no instruction): at 16 frames per workgroup the loop runs twice, and the 16 window
        // addresses and 18 twiddles hoisted out of it as loop invariants do not fit the 80 registers of six waves per SIMD
        int ln = lane;
        asm volatile("" : "+v"(ln));
        float* rr = re + f * ROWP;
        float* ii = im + f * ROWP;
        cf zv[8];
        const int s0 = (tA + f) * hop + left - NFFT / 2;      // clip sample under window position 0 (before reflection)
        float xa[8], xc[8], wa[8], wc[8];
        // interior frames: the window's samples are the contiguous run w[s0 .. s0 + win) inside the clip, one aligned 8-byte load per pair
        const bool interior = s0 >= 0 && s0 + win <= Lb && !window && !(left & 1) && !(s0 & 1) && !(wave_stride & 1) &&
                              !((uintptr_t)wave & 7);
        if (interior) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j0 = 2 * (ln + 64 * q) - left;
                const bool ok = j0 >= 0 && j0 < win;          // win even: j0 + 1 < win too
                const float2 v = ok ? *reinterpret_cast<const float2*>(w + s0 + j0) : make_float2(0.f, 0.f);
                zv[q] = cf{v.x, v.y};
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {             // all loads first (predicated), arithmetic afterwards
                const int n = ln + 64 * q;
                const int j0 = 2 * n - left, j1 = j0 + 1;
                int a0 = s0 + j0, a1 = s0 + j1;
                if (a0 < 0) a0 = -a0;
                if (a0 >= Lb) a0 = 2 * (Lb - 1) - a0;         // the reflection at the clip's own end
                if (a1 < 0) a1 = -a1;
                if (a1 >= Lb) a1 = 2 * (Lb - 1) - a1;
                const bool ok0 = j0 >= 0 && j0 < win && a0 >= 0 && a0 < Lb, ok1 = j1 >= 0 && j1 < win && a1 >= 0 && a1 < Lb;
                xa[q] = ok0 ? w[a0] : 0.f;
                xc[q] = ok1 ? w[a1] : 0.f;
                wa[q] = (window && ok0) ? window[j0] : 1.f;
                wc[q] = (window && ok1) ? window[j1] : 1.f;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) zv[q] = cf{xa[q] * wa[q], xc[q] * wc[q]};
        }
        // the twiddles are fetched once the frame's samples are in registers: live across the 32 loads above they spill
        LaneTw ltw;
        load_lane_twiddles(ln, ltw);
        fft512_wave<-1, true, false>(rr, ii, ln, ltw, zv);
        cf A[4], Bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int k = ln + 1 + 64 * q;
            A[q] = cf{rr[fidx(k)], ii[fidx(k)]};
            Bv[q] = cf{rr[fidx(512 - k)], ii[fidx(512 - k)]};
        }
        cf Z0 = cf{rr[0], ii[0]};
        wave_fence();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int k = ln + 1 + 64 * q;
            cf xk, xm;
            rfft_post_pair(A[q], Bv[q], ltw.glue[q], xk, xm);
            rr[fidx(k)] = xk.x; ii[fidx(k)] = xk.y;
            rr[fidx(512 - k)] = xm.x; ii[fidx(512 - k)] = xm.y;
        }
        if (ln == 0) {
            rr[0] = Z0.x + Z0.y; ii[0] = 0.f;
            rr[fidx(512)] = Z0.x - Z0.y; ii[fidx(512)] = 0.f;
        }
    }
    __syncthreads();

    // coalesced epilogue, t fastest; frames T_b <= t < T of this tile were not transformed (their LDS rows are unwritten): zeros
    const int nclip = Tb - tA;                        // > 0
    for (int idx = tid; idx < NBIN * FB; idx += THREADS) {
        int tl = idx & (FB - 1), k = idx / FB;
        if (tl >= nvalid) continue;
        float xr = 0.f, xi = 0.f;
        if (tl < nclip) { xr = re[tl * ROWP + fidx(k)]; xi = im[tl * ROWP + fidx(k)]; }
        long o = ((long)b * NBIN + k) * T + tA + tl;
        if (X) reinterpret_cast<float2*>(X)[o] = make_float2(xr, xi);
        if (mag) mag[o] = tl < nclip ? __builtin_sqrtf(fmaf(xr, xr, xi * xi)) : 0.f;
        if (phase) phase[o] = tl < nclip ? atan2f(xi, xr) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------ inverse
// X' = X * g(m, |X|) / |X| of the clip's frames t < T_b, mask columns >= Wm_b = min(Tm, 4 (T_b / 4)) counting as 0; grid z = branch
// (0: mask-in, 1: mask-out; which0 = 1 with one branch: mask-out only).
template <int FB>
__global__ __launch_bounds__(THREADS, 4) void istft_c64_ragged_kernel(
    const float* __restrict__ spec, const float* __restrict__ mask, const int* __restrict__ lens, int Fm, int Tm, int mode,
    int which0, float* __restrict__ out0, float* __restrict__ out1, long wave_stride, int T, int L, int hop, int win, int R,
    const float* __restrict__ window) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWP = RowPitch<FB>::value;
    float* re = smem;
    float* im = smem + FB * ROWP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, g = blockIdx.x;
    const int left = (NFFT - win) / 2;
    const int S = FB - R + 1;                         // complete hop-segments this workgroup emits
    const int tA = g * S - (R - 1);                   // first frame it transforms (may be < 0)
    const int pass = blockIdx.z;
    const int which = which0 + pass;                  // 0: mask-in, 1: mask-out
    float* out = (pass == 0 ? out0 : out1) + (long)b * wave_stride;
    const int Lb = clip_samples(lens, b, L);
    const int Tb = 1 + Lb / hop;
    const int Wm = min(Tm, 4 * (Tb / 4));             // the clip's own mask width

    const int nA = (tA + R - 1) * hop + left - NFFT / 2;       // clip sample of this workgroup's first output
    if (nA >= Lb) {                                   // every sample lies past the clip: zeros (workgroup-uniform)
        const int nE = min(L, nA + S * hop);
        for (int n = max(nA, 0) + tid; n < nE; n += THREADS) out[n] = 0.f;
        return;
    }

    constexpr int NIT = (NBIN * FB + THREADS - 1) / THREADS;
    float2 ld0[NIT];
    float ldm[NIT];
    bool valid[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * THREADS;
        const int tl = idx & (FB - 1), k = idx / FB, t = tA + tl;
        valid[it] = idx < NBIN * FB && t >= 0 && t < Tb;
        ld0[it] = make_float2(0.f, 0.f);
        ldm[it] = 0.f;
        if (valid[it]) {
            const long o = ((long)b * NBIN + k) * T + t;
            ld0[it] = reinterpret_cast<const float2*>(spec)[o];
            if (k < Fm && t < Wm) ldm[it] = mask[((long)b * Fm + k) * Tm + t];
        }
    }

    // 1. the 513 x FB tile: mask application into the LDS rows
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * THREADS;
        if (idx >= NBIN * FB) break;
        const int tl = idx & (FB - 1), k = idx / FB;
        float xr = ld0[it].x, xi = ld0[it].y;
        float m = ldm[it];
        if (which == 1) m = 1.f - m;
        const float f = valid[it] ? mask_factor(m, __builtin_sqrtf(fmaf(xr, xr, xi * xi)), mode) : 0.f;
        xr *= f; xi *= f;
        re[tl * ROWP + fidx(k)] = xr;
        im[tl * ROWP + fidx(k)] = xi;
    }
    __syncthreads();
    LaneTw ltw;
    load_lane_twiddles(lane, ltw);

    // 2. one wavefront per frame: Hermitian glue, inverse FFT512, the windowed time samples go back into the frame's own LDS rows
    static_assert(2 * RowPitch<FB>::value >= NFFT, "a frame's time samples must fit its two LDS rows");
#pragma unroll 1
    for (int f = wv; f < FB; f += THREADS / 64) {
        int t = tA + f;
        if (t < 0 || t >= Tb) continue;               // wave-uniform
        int ln = lane;                                // opaque per iteration where the loop runs twice, as in the forward
        if constexpr (FB > THREADS / 64) asm volatile("" : "+v"(ln));
        float* rr = re + f * ROWP;
        float* ii = im + f * ROWP;
        cf A[4], Bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int k = ln + 1 + 64 * q;
            A[q] = cf{rr[fidx(k)], ii[fidx(k)]};
            Bv[q] = cf{rr[fidx(512 - k)], ii[fidx(512 - k)]};
        }
        float x0 = rr[0], xn = rr[fidx(512)];
        wave_fence();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int k = ln + 1 + 64 * q;
            cf zk, zm;
            irfft_pre_pair(A[q], Bv[q], ltw.glue[q], zk, zm);
            rr[fidx(k)] = zk.x; ii[fidx(k)] = zk.y;
            rr[fidx(512 - k)] = zm.x; ii[fidx(512 - k)] = zm.y;
        }
        if (ln == 0) { rr[0] = 0.5f * (x0 + xn); ii[0] = 0.5f * (x0 - xn); }
        wave_fence();
        cf yv[8];
        fft512_wave<+1, false, true>(rr, ii, ln, ltw, yv);
        wave_fence();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = ln + 64 * q;
            const int j0 = 2 * n - left, j1 = j0 + 1;
            float a = yv[q].x * (1.f / 512.f), c = yv[q].y * (1.f / 512.f);
            if (!(left & 1)) {
                if (j0 < 0 || j0 >= win) continue;
                if (window) { a *= window[j0]; c *= window[j1]; }
                *reinterpret_cast<float2*>(j0 < ROWP ? rr + j0 : ii + (j0 - ROWP)) = make_float2(a, c);
            } else {
                if (j0 >= 0 && j0 < win) *(j0 < ROWP ? rr + j0 : ii + (j0 - ROWP)) = window ? a * window[j0] : a;
                if (j1 >= 0 && j1 < win) *(j1 < ROWP ? rr + j1 : ii + (j1 - ROWP)) = window ? c * window[j1] : c;
            }
        }
    }
    __syncthreads();

    // 3. emit the S hop-segments: sum over the clip's overlapping frames / window envelope on [0, L_b), zeros on [L_b, L)
    for (int sgm = 0; sgm < S; ++sgm) {
        const int thi = tA + R - 1 + sgm;
        const int n0 = thi * hop + left - NFFT / 2;
        for (int u = tid; u < hop; u += THREADS) {
            const int n = n0 + u;
            if (n < 0 || n >= L) continue;
            if (n >= Lb) { out[n] = 0.f; continue; }
            float env = 0.f, sum = 0.f;
            for (int r = 0; r < R; ++r) {
                const int t = thi - r, j = u + r * hop;
                if (t >= 0 && t < Tb && j < win) {
                    const float ww = window ? window[j] : 1.f;
                    env += ww * ww;
                    const int f = t - tA;             // 0 <= f < FB
                    sum += j < ROWP ? re[f * ROWP + j] : im[f * ROWP + j - ROWP];
                }
            }
            out[n] = env > 1e-11f ? sum / env : 0.f;
        }
    }
}

static size_t lds_rows_bytes(int FB) { return sizeof(float) * 2 * FB * (FB == 8 ? RowPitch<8>::value : RowPitch<16>::value); }

// advh_set_option("stft_frames_per_workgroup") lives in stft.hip; the ragged entries follow it through this mirror
static int g_fb = 8;

static int check_frame_args(const void* lens, int B, int T, int L, int hop, int win) {
    if (!lens || B <= 0 || L <= 0 || hop <= 0 || win <= 0 || win > NFFT || (win & 1) || T != 1 + L / hop) return ADVH_EINVAL;
    if (L <= NFFT / 2) return ADVH_EINVAL;           // reflect padding needs L > n_fft/2
    if (B > 65535) return ADVH_EUNSUPPORTED;          // one grid row per clip
    return ADVH_OK;
}

}  // namespace stft_ragged
}  // namespace advh

using namespace advh;
using namespace advh::stft_ragged;

int advh_stft_ragged_set_fb(int fb) { g_fb = fb; return ADVH_OK; }

int advh_init_stft_ragged() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return ADVH_ELAUNCH;
    if (stft_ragged::g_init_done[dev]) return ADVH_OK;
    static cf host[1024];
    for (int k = 0; k < 1024; ++k) {
        host[k].x = (float)cos(2.0 * M_PI * k / 1024.0);
        host[k].y = (float)sin(2.0 * M_PI * k / 1024.0);
    }
    if (hipMemcpyToSymbol(HIP_SYMBOL(stft_ragged::g_twiddle), host, sizeof(host)) != hipSuccess) return ADVH_ELAUNCH;
    const void* big[] = {(const void*)stft_fwd_ragged_kernel<16>, (const void*)stft_fwd_ragged_kernel<8>,
                         (const void*)istft_c64_ragged_kernel<16>, (const void*)istft_c64_ragged_kernel<8>};
    for (const void* f : big)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return ADVH_ELAUNCH;
    stft_ragged::g_init_done[dev] = true;
    return ADVH_OK;
}

extern "C" int advh_stft_forward_ragged(const float* wave, int64_t wave_stride, const int32_t* lens, int B, int L, int hop, int win,
                                        const float* window, float* X, float* mag, float* phase, int T, advh_stream_t stream) {
    int rc = check_frame_args(lens, B, T, L, hop, win);
    if (rc) return rc;
    if (!wave || wave_stride < L || (!X && !mag && !phase)) return ADVH_EINVAL;
    if (((uintptr_t)wave | (uintptr_t)window | (uintptr_t)mag | (uintptr_t)phase | (uintptr_t)lens) & 3 || ((uintptr_t)X & 7)) return ADVH_EINVAL;
    if (!stft_ragged::init_done_here()) return ADVH_ENOTINIT;
    const int FB = g_fb;
    dim3 grid((T + FB - 1) / FB, B);
    if (FB == 8)
        hipLaunchKernelGGL((stft_fwd_ragged_kernel<8>), grid, dim3(THREADS), lds_rows_bytes(8), (hipStream_t)stream, wave, (long)wave_stride,
                           (const int*)lens, L, hop, win, window, X, mag, phase, T);
    else
        hipLaunchKernelGGL((stft_fwd_ragged_kernel<16>), grid, dim3(THREADS), lds_rows_bytes(16), (hipStream_t)stream, wave, (long)wave_stride,
                           (const int*)lens, L, hop, win, window, X, mag, phase, T);
    return ADVH_LAUNCH_CHECK();
}

extern "C" int advh_istft_masked_c64_ragged(const float* spec, const float* mask, int Fm, int Tm, int mode, float* wave_in, float* wave_out,
                                            int64_t wave_stride, const int32_t* lens, int B, int T, int L, int hop, int win,
                                            const float* window, advh_stream_t stream) {
    int rc = check_frame_args(lens, B, T, L, hop, win);
    if (rc) return rc;
    if (!spec || !mask || wave_stride < L || Fm <= 0 || Tm <= 0 || Fm > NBIN || Tm > T || (!wave_in && !wave_out)) return ADVH_EINVAL;
    if (mode != ADVH_MASK_LINEAR && mode != ADVH_MASK_LOG1P) return ADVH_EINVAL;
    if (((uintptr_t)mask | (uintptr_t)window | (uintptr_t)wave_in | (uintptr_t)wave_out | (uintptr_t)lens) & 3 || ((uintptr_t)spec & 7)) return ADVH_EINVAL;
    const int R = (win + hop - 1) / hop;
    const int FB = g_fb;
    if (R > FB / 2) return ADVH_EUNSUPPORTED;
    if (!stft_ragged::init_done_here()) return ADVH_ENOTINIT;
    const int S = FB - R + 1, left = (NFFT - win) / 2;
    int which0 = 0, nz = 2;
    float *p0 = wave_in, *p1 = wave_out;
    if (!wave_in) { which0 = 1; p0 = wave_out; p1 = nullptr; nz = 1; }
    else if (!wave_out) { nz = 1; }
    const int nG = (NFFT / 2 + L - left + S * hop - 1) / (S * hop);
    dim3 grid(nG, B, nz);
    if (FB == 8)
        hipLaunchKernelGGL((istft_c64_ragged_kernel<8>), grid, dim3(THREADS), lds_rows_bytes(8), (hipStream_t)stream, spec, mask,
                           (const int*)lens, Fm, Tm, mode, which0, p0, p1, (long)wave_stride, T, L, hop, win, R, window);
    else
        hipLaunchKernelGGL((istft_c64_ragged_kernel<16>), grid, dim3(THREADS), lds_rows_bytes(16), (hipStream_t)stream, spec, mask,
                           (const int*)lens, Fm, Tm, mode, which0, p0, p1, (long)wave_stride, T, L, hop, win, R, window);
    return ADVH_LAUNCH_CHECK();
}
