/* libaddvisor_hip -- C ABI of the MI355X (gfx950) ADDvisor explanation hot path.
 *
 * The reference (davidcombei/xAI-Audio-Deepfakes) has no FFI: its boundary is a set of Python
 * modules whose arithmetic lives in torch / transformers.  Each entry point below replaces the
 * device work behind one of those calls; the citation says which (paths relative to the
 * reference repo, `transformers/...` = the HF package it imports).  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (hipMalloc / torch allocator),
 *     except `advh_gemm_desc` and the small parameter structs, which are host memory read
 *     during the call;
 *   - `stream` is a hipStream_t (passed as void*; NULL = the default stream); calls only
 *     enqueue work, they never synchronise, allocate or free, so they may be graph-captured;
 *   - return value: 0 = ok, <0 = ADVH_E* error (no exceptions cross the ABI, nothing is printed);
 *   - no global state except immutable tables (FFT twiddles) built by advh_init();
 *   - thread-compatible: concurrent calls must use different streams and buffers.
 */
#ifndef ADDVISOR_HIP_H
#define ADDVISOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* advh_stream_t;

enum {
    ADVH_OK = 0,
    ADVH_EINVAL = -1,   /* bad argument (shape, alignment, null pointer)            */
    ADVH_ELAUNCH = -2,  /* hipLaunchKernel / hipGetLastError reported a failure     */
    ADVH_ENOTINIT = -3, /* advh_init() has not been called on this device          */
    ADVH_EUNSUPPORTED = -4
};

/* Library / build identification: returns a static NUL-terminated string ("gfx950 ..."). */
const char* advh_version(void);

/* Build the immutable device tables (FFT twiddles) on the current device and raise the dynamic-LDS
 * limits of the kernels that need more than 64 KiB.  Call once per process and device, outside
 * any stream capture.  Idempotent. */
int advh_init(void);

/* Tuning knobs (process-wide, not thread-safe; set before launching work):
 *   "stft_frames_per_workgroup" = 8 (default) | 16 : STFT / ISTFT frames per workgroup.
 *   "attention_bwd_mfma_f32" = 0 (default) | 1 : advh_attention_bwd_split on the fp32-input matrix instruction for every
 *       head dim (1) instead of the split-arithmetic kernel for head dims <= 64 (0); same results to 1e-6 (A/B runs). */
int advh_set_option(const char* name, int value);

/* ---------------------------------------------------------------------------------------------
 * STFT  -- replaces AudioProcessor.compute_stft (audioprocessor.py:82-112):
 *   pad/crop to L samples, torch.stft(n_fft=1024, hop, win, window=None|window, center=True,
 *   pad_mode="reflect", onesided) -> X, |X|, angle(X).
 * wave   [B][wave_stride] fp32, n_in valid samples per clip (n_in < L: zero-padded tail,
 *        n_in > L: cropped);  window: NULL = rectangular `win`-long window, else `win` floats.
 * X      [B][513][T][2] fp32 (complex64, t fastest) or NULL;  mag, phase [B][513][T] or NULL.
 * T must equal 1 + L / hop.  n_fft is fixed at 1024 (the only size the reference uses).        */
int advh_stft_forward(const float* wave, int64_t wave_stride, int n_in, int B, int L, int hop, int win,
                      const float* window, float* X, float* mag, float* phase, int T, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Masked ISTFT -- replaces, fused in one kernel, the mask application + polar recombination of
 *   loss_function.py:36-45 (mode ADVH_MASK_LINEAR) / LMAC_metrics.py:136-153 (ADVH_MASK_LOG1P)
 *   and AudioProcessor.compute_invert_stft (audioprocessor.py:117-131: torch.istft, length=L).
 * mag, phase [B][513][T] fp32;  mask [B][Fm][Tm] fp32 (the U-Net output; bins outside the
 *   Fm x Tm crop count as mask = 0) or NULL with ADVH_MASK_NONE.
 * wave_in  <- istft( g(mask)   * e^{j phase} ),  wave_out <- istft( g(1-mask) * e^{j phase} );
 *   either may be NULL.  [B][wave_stride], L samples written per clip.                         */
enum { ADVH_MASK_NONE = 0, ADVH_MASK_LINEAR = 1, ADVH_MASK_LOG1P = 2 };
int advh_istft_masked(const float* mag, const float* phase, const float* mask, int Fm, int Tm, int mode,
                      float* wave_in, float* wave_out, int64_t wave_stride, int B, int T, int L, int hop,
                      int win, const float* window, advh_stream_t stream);

/* Same resynthesis from the COMPLEX spectrogram X [B][513][T][2] (advh_stft_forward's X) instead of (|X|, angle X):
 * X' = X * g(mask, |X|) / |X|, which equals g e^{j angle X} of loss_function.py:36-45 / LMAC_metrics.py:136-153 without the
 * atan2 / sincos round trip (more accurate, and no transcendental per bin in the linear domain).  mode: LINEAR or LOG1P. */
int advh_istft_masked_c64(const float* spec, const float* mask, int Fm, int Tm, int mode, float* wave_in, float* wave_out,
                          int64_t wave_stride, int B, int T, int L, int hop, int win, const float* window,
                          advh_stream_t stream);

/* Plain ISTFT of a complex64 spectrogram [B][513][T][2] (audioprocessor.py:117-131). */
int advh_istft_c64(const float* spec, float* wave, int64_t wave_stride, int B, int T, int L, int hop, int win,
                   const float* window, advh_stream_t stream);

/* Band-swap resynthesis (the data generator of hifigan.py:196-228 and train_logReg_swapping.py:64-92; SURVEY.md §8(f)
 * rank 2): for band z in [0, nbands) the bins [k0 + z*kw, k0 + (z+1)*kw) of the complex64 spectrogram spec_a
 * [B][513][T] are replaced by those of spec_b and the result is inverted (torch.istft semantics as advh_istft_c64);
 * waves [nbands][B][L], band stride band_stride >= B*wave_stride elements.  One launch, grid z = band.            */
int advh_istft_bandswap(const float* spec_a, const float* spec_b, int k0, int kw, int nbands, float* waves,
                        int64_t wave_stride, int64_t band_stride, int B, int T, int L, int hop, int win,
                        const float* window, advh_stream_t stream);

/* Backward of advh_istft_masked from ONE resynthesised waveform to the mask (LMACLoss backward,
 * loss_function.py:36-47 / SURVEY.md §8(f) rank 1): g_wave = dL/d wave [B][L] (row stride g_stride), which = 0 for
 * the mask-in branch (a = m M), 1 for mask-out (a = (1 - m) M); dmask [B][Fm][Tm] is overwritten.  `mask` is only
 * read in ADVH_MASK_LOG1P mode.  Adjoint of torch.istft: divide by the window envelope, zero-extend, frame with the
 * synthesis window, rfft, scale by c_k / n_fft.                                                                    */
int advh_istft_masked_bwd(const float* g_wave, int64_t g_stride, const float* mag, const float* phase, const float* mask,
                          int Fm, int Tm, int mode, int which, float* dmask, int B, int T, int L, int hop, int win,
                          const float* window, advh_stream_t stream);

/* The row-mapped pair of the mask-domain attributions (addvisor_hip/spectral_attribution.py): `rows` masks [rows][Fm][Tm] over
 * the spectrograms spec [B][513][T][2] of B clips, mask-in branch only.  Launch row r reads the spectrogram of clip
 *   c = (row0 + r) % B  (clip_major = 0: rows s * B + b, k * B + b, (p * K + j) * B + b)  or
 *   c = (row0 + r) / S  (clip_major = 1: rows b * S + s),
 * clamped to [0, B): the clip comes from the rule, no index array goes to the device.  S >= 1 in both rules.
 * advh_istft_masked_rows     : wave [rows][wave_stride] <- istft(X_c * g(mask_r, |X_c|) / |X_c|), the arithmetic of
 *                              advh_istft_masked_c64's mask-in signal.
 * advh_istft_masked_rows_bwd : dmask [rows][Fm][Tm] (overwritten) from g_wave [rows][g_stride], the adjoint of the above down to
 *                              the mask, read from the complex X (no sincos):  linear dm = sc (Re G Re X + Im G Im X), the imaginary
 *                              term dropped on bins 0 and 512;  log1p dm = log1p(M) exp(m log1p(M)) da with cos, sin = X / M, and
 *                              0 where M < 1e-12.  `mask` is read in ADVH_MASK_LOG1P mode only (NULL allowed otherwise).
 * Argument errors return a negative code before any HIP call.                                                        */
int advh_istft_masked_rows(const float* spec, const float* mask, int Fm, int Tm, int mode, float* wave, int64_t wave_stride,
                           int rows, int64_t row0, int clip_major, int S, int B, int T, int L, int hop, int win,
                           const float* window, advh_stream_t stream);
int advh_istft_masked_rows_bwd(const float* g_wave, int64_t g_stride, const float* spec, const float* mask, int Fm, int Tm,
                               int mode, float* dmask, int rows, int64_t row0, int clip_major, int S, int B, int T, int L,
                               int hop, int win, const float* window, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Implicit GEMM on the matrix cores (fp16 operands, fp32 accumulate):
 *
 *     out[row(m) + col(n)] = act( sum_k A(m,k) * W[n][k] + bias[n] ) + resid[row(m) + col(n)]
 *
 * replaces the cuDNN / cuBLAS calls behind nn.Conv1d, nn.Linear (transformers/models/wav2vec2/
 * modeling_wav2vec2.py:254-572) and nn.Conv2d / nn.ConvTranspose2d (addvisor.py:12-84).
 * Activations are channels-last fp16; a convolution tap is a constant offset from the row's base
 * address, listed per 16-byte K-chunk in `ktab`.
 *
 * Row enumeration: m = (b*Hg + h)*Wg + w, 0 <= m < M.  Rows with (h,w) outside the window
 * [h0,h1) x [w0,w1) are "halo" rows: they read a safe in-window row and, if `halo_zero`, have
 * zeros written (so a zero-haloed NHWC output map is produced complete by one launch).
 * A row base, in 16-byte chunks (8 halfs):  b*a_sB[s] + h*a_sH[s] + w*a_sW[s] + a_c0[s]  (source s).
 * K-chunk c (0 <= c < Ktot/8) reads 8 halfs at  A_s + 8*(rowbase_s + (ktab[c] & 0x7fffffff)),
 * s = ktab[c] >> 31.  Ktot % 64 == 0; padding chunks must pair zero weights with any readable chunk.
 * W is [w_rows][Ktot] fp16, w_rows >= N rounded up to the tile's BN (extra rows are read, never used).
 * Output element offset: b*o_sB + h*o_sH + w*o_sW + o_c0 + (n / n_div)*o_sNhi + n % n_div + z*o_sZ
 * (n_div % 4 == 0; every term a multiple of 4 elements).  `nz` batches (grid z) advance the
 * operands by a_sZ (chunks), w_sZ (elements), bias_sZ, o_sZ.                                     */
enum { ADVH_ACT_NONE = 0, ADVH_ACT_GELU = 1, ADVH_ACT_LEAKY = 2 };
enum { ADVH_TILE_AUTO = 0, ADVH_TILE_128x128 = 1, ADVH_TILE_256x64 = 2, ADVH_TILE_256x32 = 3,
       ADVH_TILE_256x128_W8 = 9, ADVH_TILE_128x256_W8 = 10 /* 512-thread instances of the same single-buffer kernel, 64x64 wave tiles, 2 workgroups
                                                               per CU: tuner candidates (they win one K = 4096 shape); fp16 operands only */ };

typedef struct advh_gemm_desc {
    const void* A0;       /* fp16 source 0                                   */
    const void* A1;       /* fp16 source 1 (skip-concat by pointer) or NULL  */
    const void* W;        /* fp16 [nz][w_rows][Ktot]                         */
    const int32_t* ktab;  /* [Ktot/8] chunk offsets, bit 31 selects A1       */
    const float* bias;    /* fp32 [nz][N] or NULL                            */
    const void* resid;    /* residual, addressed like out, or NULL           */
    void* out_h;          /* fp16 output or NULL                             */
    void* out_f;          /* fp32 output or NULL                             */
    int32_t M, N, Ktot, w_rows;
    int32_t Hg, Wg, h0, h1, w0, w1, halo_zero;
    int64_t a_sB[2], a_sH[2], a_sW[2], a_c0[2], a_sZ[2];
    int64_t w_sZ, bias_sZ;
    int64_t o_sB, o_sH, o_sW, o_c0, o_sNhi, o_sZ;
    int32_t n_div, nz;
    int32_t act;          /* ADVH_ACT_*                                      */
    float slope;          /* LeakyReLU slope                                 */
    int32_t resid_f32;    /* 1: resid is fp32, 0: fp16                       */
    int32_t ktab_identity;/* 1: ktab[c] == c for all c (plain GEMM rows): kernels may skip the lookup */
    void* out_h2;         /* optional second fp16 output = LeakyReLU_{slope2}(value written to out_h):
                             the pre-activated copy the next HiFi-GAN conv consumes (ResBlock1)          */
    float slope2;
    /* ConvTranspose1d by phase decomposition (stride r = ph_r > 0): column block n / n_div is the output phase,
       row w the input position; the element is written only if 0 <= w*ph_r + n/n_div - ph_pad < ph_T.   */
    int32_t ph_r, ph_pad, ph_T;
    /* backward support (input-gradient chain of the frozen embedder, captum_saliency.py:131-135):
       out_pre: fp16 copy of the value BEFORE `act` (saved for the activation derivative), or NULL;
       dact_src: fp16 tensor addressed like out; if set, the value is multiplied by GELU'(dact_src[o])
       (after bias, before resid): turns a dgrad GEMM's output into the gradient w.r.t. the previous
       layer's pre-activation.                                                                          */
    void* out_pre;
    const void* dact_src;
    /* wide = 1: the rows of W are packed permuted inside every 32-row block -- packed row R holds output channel
       32 (R>>5) + 8 ((R>>2)&3) + 4 ((R>>4)&1) + (R&3) -- so that a lane's accumulators are 8 consecutive channels and
       the epilogue moves 16 bytes of fp16 per lane.  Requires N, n_div, o_c0 and every o_s* stride (o_sB, o_sH, o_sW, o_sNhi,
       o_sNhh, o_sZ, o_sZ2) % 8 == 0: checked on the host, ADVH_EINVAL otherwise (a lane stores 8 columns, so N % 8 == 4 would
       write past N).  wide = 0: packed row R is channel R.                                                 */
    int32_t wide;
    /* row pitch of W in elements; 0 = Ktot.  Lets a launch (or grid-z batch) reduce over a K-slice of a wider
       K-major matrix: the split-K weight-gradient GEMMs of the U-Net training step.                       */
    int64_t w_ld;
    /* super-column width in N tiles for the 256-thread kernels' tile order (0 = plain row-major order): all M tiles of
       `sc` N-tiles are walked before the next `sc`, keeping that weight slice L2-resident.                     */
    int32_t sc;
    /* second level of the column -> address split (ConvTranspose2d with all kh*kw sub-pixels in ONE launch): with
       q = n / n_div, the offset is (q / n_sub)*o_sNhh + (q % n_sub)*o_sNhi instead of q*o_sNhi; n_sub <= 1 = off. */
    int32_t n_sub;
    int64_t o_sNhh;
    /* two-level grid-z batch (every tile, the 512-thread ones included: they are instances of the same kernel): with nz_lo > 1
       the batch index z in [0, nz) splits into zh = z / nz_lo, zw = z % nz_lo and the operands advance by
       a_sZ*zh + a_sZ2*zw (chunks) and o_sZ*zh + o_sZ2*zw (elements); W and bias still advance by w_sZ*z, bias_sZ*z.
       The four output-parity classes of a fused ConvTranspose2d(2,2)+Conv2d launch are such a batch.
       z_inner = 1: the nz batches of one tile are dispatched next to each other (z fastest in the workgroup order)
       instead of batch after batch, so batches that read the same operand rows meet in L2.                  */
    int32_t nz_lo, z_inner;
    int64_t a_sZ2[2];
    int64_t o_sZ2;
    /* plain = 1 (requires ktab_identity and one source): every row m in [0, M) -- valid or not -- may be read at chunk
       a_c0[0] + m * a_sW[0] (+ z * a_sZ[0]), K contiguous chunks; a_sB / a_sH / the window are then used for the OUTPUT
       addressing only.  Lets the 128x128 tile run its affine-row loader (Linear layers, feature-encoder Conv1d: the
       caller guarantees that the last row's K chunks are inside the allocation).  The fp16 tiles without an affine-row
       loader (256x64, 256x32 and the 512-thread ones; in split mode every tile has one) serve plain = 1 with the gathered
       loader, which addresses valid rows by b*a_sB + h*a_sH + w*a_sW: a_sH must equal Wg*a_sW and a_sB must equal Hg*Wg*a_sW
       (or the grid is one line / one item) so that both rules name the same chunk.                                 */
    int32_t plain;
    /* plain_out = 1 (with plain): every row is valid (the window is the whole grid), output row m starts at
       o_c0 + m * o_sW + the batch offset and the columns are one block (n_div >= N, no phases, no sub-pixel split):
       the epilogue skips the row decomposition and the column divisions.                                          */
    int32_t plain_out;
    /* split = 1: fp32-class mode.  Every fp16 operand and fp16 output is a PAIR of planes (hi, lo) in the split format
       x = hi + lo * 2^-11 (csrc/device_math.h: hi = fp16(x), lo = fp16((x - hi) * 2^11)); the lo plane of source s starts
       a_lo[s] chunks behind A_s, that of W w_lo elements behind W, that of out_h / out_h2 / a fp16 resid o_lo elements
       behind the hi plane, all addressed like the hi plane.  The kernel issues three MFMAs per fragment pair
       (Wh*Ah + (Wh*Al + Wl*Ah) * 2^-11, fp32 accumulate): the arithmetic class of the reference's fp32 layers.
       Tiles: 128x128, 256x64, 256x32 (AUTO picks as for fp16; the 512-thread tiles return ADVH_EUNSUPPORTED); out_pre /
       dact_src are plane pairs like out_h (the fp32-class gradient chain of the embedder uses them).               */
    int32_t split;
    int64_t a_lo[2];
    int64_t w_lo;
    int64_t o_lo;
} advh_gemm_desc;

int advh_gemm_f16(const advh_gemm_desc* desc, int tile, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * wav2vec2 waveform front end -- replaces zero_mean_unit_var_norm (classifier_embedder.py:59-63)
 * and feature-encoder layer 0 (Conv1d(1,C0,10,stride 5) [+ GroupNorm(C0,C0) + GELU],
 * transformers/models/wav2vec2/modeling_wav2vec2.py:254-323) behind AudioProcessor.extract_features
 * (audioprocessor.py:69-77).
 * wave [B][wave_stride] fp32 (n_in valid samples, padded / cropped to L);  w0 [C0][10] fp32.
 * mode 0 ("group"): out = GELU(GroupNorm(conv)), gamma/beta [C0];  mode 1 ("layer"): out = conv + bias0.
 * out: fp16 channels-last [B][P0][C0], rows t in [T0,P0) written as zeros; T0 = (L-10)/5 + 1.
 * normalize: 1 = apply zero_mean_unit_var_norm first; 0 = wave is already normalised (the raw
 *   `wav2vec2(input_values)` call of audioprocessor.py:76).
 * stats_ws: [B][2] fp32 workspace (clip mean, 1/(std+1e-7));  norm_ws: [B][C0][2] fp32 (mode 0);
 * mr_ws: NULL, or [B][C0][2] fp32 <- per-channel (mean, rstd) of the GroupNorm, kept for the backward.  */
int advh_w2v2_frontend(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                       const float* bias0, const float* gamma, const float* beta, int mode, int normalize, float* stats_ws,
                       float* norm_ws, float* mr_ws, void* out, int T0, int P0, int C0, advh_stream_t stream);

/* LayerNorm over the last dimension (+ optional GELU): nn.LayerNorm call sites of
 * modeling_wav2vec2.py:275-299, 422-434, 575-654, 689-802.  in: [M][in_ld] fp32 (in_is_f32) or fp16;
 * out_f (fp32) and/or out_h (fp16), row stride out_ld.  C % 4 == 0, C <= 2048. */
int advh_layernorm(const void* in, int in_is_f32, int64_t in_ld, const float* gamma, const float* beta,
                   float* out_f, void* out_h, int64_t out_ld, int M, int C, float eps, int gelu,
                   advh_stream_t stream);
/* Same with an fp16 addend row: y = LayerNorm(in + add_h) -- the residual add of a post-LN encoder layer
 * (modeling_wav2vec2.py:689-726: hidden = attn_residual + attention(...); layer_norm(hidden)) fused into the LayerNorm, so
 * the projection before it stores only its fp16 result instead of reading and re-writing the fp32 stream.  add_h NULL =
 * advh_layernorm. */
int advh_layernorm_add(const void* in, int in_is_f32, int64_t in_ld, const void* add_h, int64_t add_ld, const float* gamma,
                       const float* beta, float* out_f, void* out_h, int64_t out_ld, int M, int C, float eps, int gelu,
                       advh_stream_t stream);

/* Operand gather of the grouped positional Conv1d (modeling_wav2vec2.py:326-379):
 * h [B][T][H] fp32 -> xg [G][B][T+K][H/G] fp16, data in rows [pad_left, pad_left+T), zeros elsewhere
 * (forward: pad_left = K/2; input-gradient pass: K/2 - 1 and h is multiplied by GELU'(dact_src), fp16 [B][T][H]). */
int advh_posconv_gather(const float* h, void* xg, int B, int T, int H, int G, int K, int pad_left, const void* dact_src,
                        advh_stream_t stream);

/* The grouped positional convolution itself as an LDS line-tile launch (csrc/posconv_tile.hip): one workgroup per
 * (group, clip) stages the clip's gathered rows once and streams the group's weights through an LDS ring.
 *   xg    [G][B][T+K][H/G] fp16 from advh_posconv_gather (pad_left = K/2)
 *   W     fp16 [G][K*(H/G)/32 k-steps][H/G rows][32]: weight-norm-folded conv weight [n][tap][ci] of each group, cut
 *         into 32-deep k-steps in (tap, ci) order
 *   out[b][t][c] = resid[b][t][c] + GELU(conv + bias[c])   fp32 [B][T][H] (out may alias resid).
 * Supported: K = 128, H/G in {48, 64}, T <= 256 (ADVH_EUNSUPPORTED otherwise: use the implicit GEMM).         */
typedef struct advh_posconv_desc {
    const void* xg;
    const void* W;
    const float* bias;
    const float* resid;
    float* out;
    int B, T, H, G, K;
} advh_posconv_desc;
int advh_posconv_tile_f16(const advh_posconv_desc* d, advh_stream_t stream);
int advh_posconv_tile_lds_bytes(int Cg, int T);   /* -1 = unsupported geometry */

/* softmax(Q K^T / sqrt(d)) V without mask (modeling_wav2vec2.py:438-548), T <= 256, d in {32, 64}.
 * qkv [B*T][3H] fp16 (q | k | v), ctx [B*T][H] fp16. */
int advh_attention_f16(const void* qkv, void* ctx, int B, int T, int H, int heads, advh_stream_t stream);

/* Time mean-pool + logistic regression head: LMAC_metrics.py:130 pooling + TorchLogReg.forward
 * (classifier_embedder.py:34-38).  h [B][T][H] fp32 -> logit[B], prob[B] (and pooled [B][H] if not NULL). */
int advh_pool_logreg(const float* h, const float* coef, float intercept, float* logit, float* prob,
                     float* pooled, int B, int T, int H, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * U-Net layers that are not GEMM-shaped (addvisor.py:27-84).  mag is torch's [B][Fq][Tq] fp32; the
 * H x W crop is taken by indexing.  NHWC maps are fp16 with a zero halo (PH, PW).
 * advh_unet_stem : e1.block.0 Conv2d(1,32,(5,3),stride (2,1),pad (2,1)) + folded BN + LeakyReLU;
 *                  wgt [32][15], out [B][H/2+2PH][W+2PW][32] (interior written).
 * advh_unet_pack_x: channels [c0,c0+8) of the C-channel d1 concat map <- (mag, 1, 0 x6)  (addvisor.py:79); the 1 is
 *                  the in-image indicator the fused ConvTranspose2d+Conv2d launch multiplies up1's bias with.
 * advh_unet_head : mask_head Conv2d(32,1,1) + Sigmoid -> mask (and pre-sigmoid logits) [B][H][W] fp32. */
int advh_unet_stem(const float* mag, int Fq, int Tq, int B, int H, int W, const float* wgt, const float* bias,
                   void* out, int PH, int PW, float slope, advh_stream_t stream);
int advh_unet_pack_x(const float* mag, int Fq, int Tq, int B, int H, int W, void* cat, int C, int c0, int PH, int PW,
                     advh_stream_t stream);
int advh_unet_head(const void* y, int B, int H, int W, int PH, int PW, const float* wgt, float bias, float* mask,
                   float* logits, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LMAC faithfulness metrics -- replaces compute_faithfulness / compute_fidelity / compute_AD /
 * compute_AI / compute_AG and their dataset means (LMAC_metrics.py:31-73, 164-172).
 * predictions, theta_out, masked_predictions: [n] fp32 probabilities (clean, mask-in, mask-out).
 * sums6 <- {sum faithfulness, sum fidelity, sum AD, sum AI, sum AG, n} in fp64, fixed summation
 * order; per_clip (or NULL) <- [5][n] fp32 per-clip values. */
int advh_lmac_metrics_accumulate(const float* predictions, const float* theta_out, const float* masked_predictions,
                                 int n, double* sums6, float* per_clip, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * HiFi-GAN V1 generator -- replaces hifi_gan.decode_batch (hifigan.py:106-110, 180; SpeechBrain HIFIGAN,
 * architecture of Kong et al. 2020 config V1) and the mel front end (hifigan.py:163-178).
 * The Conv1d / ConvTranspose1d layers are advh_gemm_f16 launches (plans in addvisor_hip/gemm.py); these are
 * the remaining pieces.  Maps are zero-haloed channels-last fp16 [B][T+2*halo][C].
 * advh_hifigan_pack_mel : mel [B][C][T] fp32 -> map interior.
 * advh_hifigan_mrf_mix  : y = LeakyReLU_slope((a+b+c)/3) over `numel` fp16 elements (the MRF average + the
 *                         activation in front of the next upsampler / conv_post).
 * advh_hifigan_conv_post: Conv1d(C,1,k,"same") + tanh -> wav [B][1][T] fp32; w is [k][C] fp32.
 * advh_mel_log          : out [B][n_mels][T] = log(clamp(fb^T |X|, 1e-5)), fb [F][n_mels], mag [B][F][T].     */
int advh_hifigan_pack_mel(const float* mel, void* out, int B, int C, int T, int halo, advh_stream_t stream);
/* Fidelity options of the SpeechBrain wrapper behind hifigan.py:106-110, 180 (not verifiable offline, hence options):
 * advh_hifigan_pack_mel_pad : as pack_mel with `pad` replicated frames on both sides (the generator's `inference_padding`:
 *                             F.pad(mel, (pad, pad), "replicate")); the map holds T + 2*pad interior rows.
 * advh_halo_fill_f16        : fill the halo of a channels-last fp16 map [B][T+2*halo][C] with zeros (mode 0) or with the
 *                             reflection of the interior about its first / last sample (mode 1: torch "reflect" padding, the
 *                             default padding_mode of SpeechBrain's Conv1d), so "same" convolutions read it in place.      */
int advh_hifigan_pack_mel_pad(const float* mel, void* out, int B, int C, int T, int pad, int halo, advh_stream_t stream);
int advh_halo_fill_f16(void* x, int B, int T, int C, int halo, int mode, advh_stream_t stream);
int advh_hifigan_mrf_mix(const void* a, const void* b, const void* c, void* y, float slope, int64_t numel, advh_stream_t stream);
int advh_hifigan_conv_post(const void* x, const float* w, float bias, float* wav, int B, int C, int T, int halo, int k,
                           advh_stream_t stream);
int advh_mel_log(const float* mag, const float* fb, float* out, int B, int F, int T, int n_mels, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input-gradient chain of the frozen embedder -- what captum.attr.{Saliency, InputXGradient,
 * IntegratedGradients}(Wav2vec2LogReg) obtain from autograd (captum_saliency.py:84-100, 116-135).
 * Dense products are advh_gemm_f16 launches with transposed weights (dact_src / out_pre above); these are
 * the remaining pieces.  Gradients are fp16 between GEMMs, multiplied by a power-of-two loss scale.
 *
 * advh_layernorm_bwd : dx of y = LN(x)*gamma+beta [then GELU if gelu_fwd] given dy; optionally times
 *                      GELU'(dact_src) and plus `add`; out_f (fp32) and/or out_h (fp16), all [M][C]; with
 *                      remap_P > 0 output row b*remap_T + t is written at row b*remap_P + t.
 * advh_attention_bwd_f16 : dqkv [B*T][3H] from qkv and dctx [B*T][H] (fp16); head dim a multiple of 8 up to 128;
 *                      T <= 256, but T <= 208 for head dims above 64 (the whole-clip tiles of a wider head need more
 *                      than the 160 KiB of LDS): ADVH_EUNSUPPORTED otherwise, dqkv untouched.
 * advh_pool_logreg_bwd   : dh[b][t][:] = coef * dlogit[b] / T  (fp32 and/or fp16).
 * advh_w2v2_frontend_bwd_group : dz0 [B][P0][C0] fp16 from dy0 for the GroupNorm front end (z0 recomputed).
 * advh_wave_bwd      : g [B][P0][16] fp32 (= dz0 . w0, columns 0..9) -> dx [B][dx_stride] through the
 *                      stride-5 overlap and the normaliser's Jacobian; multiplied by out_scale (1/loss scale).
 * advh_scale_rows    : y[r][:] = alpha[r] * x[r % x_rows][:] (+ y): IG path points and step accumulation.   */
int advh_layernorm_bwd(const void* x, int x_is_f32, const void* dy, int dy_is_f32, const float* gamma, const float* beta,
                       int gelu_fwd, const float* add, const void* dact_src, float* out_f, void* out_h, int M, int C,
                       float eps, int remap_T, int remap_P, advh_stream_t stream);
int advh_attention_bwd_f16(const void* qkv, const void* dctx, void* dqkv, int B, int T, int H, int heads, advh_stream_t stream);
int advh_pool_logreg_bwd(const float* coef, const float* dlogit, float* dh, void* dh16, int B, int T, int H, advh_stream_t stream);
int advh_w2v2_frontend_bwd_group(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                 const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                 const void* dy0, float* part_ws, float* sums_ws, void* dz0, int T0, int P0, int C0,
                                 advh_stream_t stream);
int advh_wave_bwd(const float* g, const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* stats_ws,
                  float* dxhat_ws, float* part_ws, int normalize, float out_scale, float* dx, int64_t dx_stride, int T0, int P0,
                  advh_stream_t stream);
int advh_scale_rows(const float* x, int x_rows, const float* alpha, float* y, int rows, int64_t n, int accumulate,
                    advh_stream_t stream);
/* advh_attr_finalize : out = |g| (mode 0, captum Saliency) or x * g (mode 1, InputXGradient / IG with zero baseline).
 * advh_time_mask     : mask[b] = |attr[b]| / (max|attr[b]| + 1e-8) (captum_saliency.py:136-139) and, if wave is
 *                      given, wave_in = wave*mask, wave_out = wave*(1-mask) (:141-143); all [B][n] fp32.          */
int advh_attr_finalize(const float* g, const float* x, float* out, int mode, int64_t total, advh_stream_t stream);
int advh_time_mask(const float* attr, float* mask, float* wave_in, float* wave_out, const float* wave, int B, int64_t n,
                   advh_stream_t stream);

/* Baseline-aware attributions (csrc/attribution_paths.hip): IntegratedGradients with a baseline and any Riemann / Gauss-Legendre
 * rule, and GradientShap (= SmoothGrad noise tunnel over InputBaselineXGradient).  The B * S expanded rows g of one attribution
 * are either step-major (IG: clip(g) = g % B) or clip-major (GradientShap: clip(g) = g / S); a chunk is the rows
 * [row0, row0 + rows).  Expanded row g has the noisy input x~ = x[clip(g)] + sigma * N(seed, g, :) (no noise is generated when
 * sigma = 0) and the baseline b = base[bidx[g]] (bidx != NULL), else base[clip(g)] (base_rows == B) or base[0]
 * (base_rows == 1).  bidx, alpha and w hold one entry per expanded row (B * S, indexed by g); an index outside
 * [0, base_rows) yields NaN for that row's values (the attribution's finiteness check reports it).  All rows [.][n] fp32.
 * Determinism: the noise of (g, j) depends on (seed, g, j) only, sums run in a fixed order, no atomics.
 *
 * advh_attr_path_points : out[r] = b + alpha[g] * (x~ - b), g = row0 + r ([rows][n]).
 * advh_attr_path_accumulate, one launch per chunk; each clip's rows of the chunk are added in global-row order:
 *   mode 0 (IG, step-major)     : total[c] += w[g] * grad[r]
 *   mode 1 (SHAP, clip-major)   : total[c] += (x~ - b) * grad[r]    (x~ recomputed from the counter, never stored)
 *   mode 2 (SHAP, clip-major)   : total[c] += grad[r]               (multiply_by_inputs = False)
 *   modes 1, 2 with row_sum != NULL also write row_sum[g] = sum_j (x~ - b)_j * grad[r]_j (GradientShap's per-sample delta).
 *   finalize, row0 = 0, rows = B, grad = the accumulated total, total = the attribution written:
 *   mode 3 : out[c] = (x[c] - b) * total[c] (IG; bidx must be NULL), row_sum[c] = sum_j out[c][j] if row_sum != NULL
 *   mode 4 : out[c] = total[c] / S (GradientShap's mean over samples; S = 1 copies the sum).
 * advh_philox_normal    : out[r][j] = N(seed, row0 + r, j): Philox4x32-10 (Salmon et al., SC'11), key = seed, counter =
 *                         (j / 4, row lo 32, row hi 32, 0); u = (2 * (word >> 9) + 1) * 2^-24; Box-Muller on the word pairs
 *                         (0, 1), (2, 3): z = sqrt(-2 ln u_a) * (cos, sin)(2 pi u_b) -- the exact noise the two kernels above add.
 *                         raw = 1 writes word j % 4 of counter (j / 4, row) instead (its bit pattern in the fp32 slot).
 * Replaces captum.attr.IntegratedGradients(baselines=..., method=...) and captum.attr.GradientShap (captum_saliency.py:3). */
typedef struct advh_path_desc {
    const float* x;        /* [B][n] inputs                                                     */
    const float* base;     /* [base_rows][n] baselines                                          */
    const int32_t* bidx;   /* [B * S] baseline row per expanded row, or NULL                    */
    int64_t n;
    uint64_t seed;
    int B, S, base_rows;
    int clip_major;        /* 0: step-major (IG), 1: clip-major (GradientShap)                   */
    float sigma;           /* >= 0                                                              */
} advh_path_desc;
int advh_attr_path_points(const advh_path_desc* d, const float* alpha, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_attr_path_accumulate(const advh_path_desc* d, const float* grad, const float* w, int mode, int64_t row0, int rows,
                              float* total, float* row_sum, advh_stream_t stream);
int advh_philox_normal(uint64_t seed, int64_t row0, int rows, int64_t n, int raw, float* out, advh_stream_t stream);

/* NoiseTunnel (csrc/attribution_paths.hip): Captum's SmoothGrad / SmoothGrad-squared / VarGrad over any attribution of the
 * [B][n] inputs x, restated (captum is absent).  S samples per clip, processed in partitions of p' consecutive samples
 * [s0, s0 + p'); a partition's rows are clip-major, row b * p' + s' (Captum's repeat_interleave), and hold
 * x~ = x[b] + sigma * N(seed, g, :) with the global counter g = b * S + s0 + s': advh_attr_path_points with base 0 (one row),
 * alpha 1 and clip_major = 1 writes them exactly (rows [b * S + s0, b * S + s0 + p') per clip), so the noise of a sample does
 * not depend on the partitioning.  The wrapped method attributes those rows; a = its fp32 attribution of one row.
 *
 * advh_nt_fold     : sum[b][j] += a, sumsq[b][j] += a * a over the partition's p rows of clip b (attr [B * p][n], row b * p + s),
 *                    in fp64, in increasing s, one thread per (b, j), no atomics: a fixed seed gives bit-identical sums.
 *                    sum and sumsq ([B][n] fp64) start at zero before the first partition.
 * advh_nt_finalize : out [B][n] fp32 from the sums over all S samples, m = sum / S, m2 = sumsq / S (fp64):
 *                    nt_type 0 (smoothgrad) m, 1 (smoothgrad_sq) m2, 2 (vargrad) m2 - m * m (not clamped, as Captum).
 * NaN / inf in attr propagate into the sums and the output (the caller's finiteness check reports them).  Null pointers,
 * B, p, n or S <= 0, and an nt_type outside [0, 2] return ADVH_EINVAL before any HIP call.
 * Replaces captum.attr.NoiseTunnel(method).attribute(x, nt_type=..., nt_samples=..., stdevs=...). */
int advh_nt_fold(const float* attr, int B, int p, int64_t n, double* sum, double* sumsq, advh_stream_t stream);
int advh_nt_finalize(const double* sum, const double* sumsq, int B, int64_t n, int S, int nt_type, float* out, advh_stream_t stream);

/* Layer attributions (csrc/attribution_layer.hip): Captum's LayerActivation, LayerGradientXActivation,
 * LayerIntegratedGradients, LayerConductance and InternalInfluence at hidden_states[l] of the encoder, restated (captum is
 * absent).  The encoder chain is started at a layer (EmbedderGrad.forward_from) and its backward stopped at one
 * (EmbedderGrad.backward(to_layer=l)); these kernels are the two ends.  All rows [.][n] fp32, contiguous.  One thread per
 * element, every product, difference and sum rounded on its own, sums in increasing step order, row sums a fixed-shape tree in
 * one workgroup, no atomics: equal inputs give equal bits for every chunking.
 *
 * advh_layer_inject : resid[r] = src[r] ([rows][n], rows = clips * T, n = H: the residual stream at the layer) and, if op != NULL,
 *     the GEMM operand copy of the same fp32 values the post-LN layer reads: one fp16 plane (split = 0) or the split format's
 *     hi plane at op and lo plane op_lo elements behind (split = 1; op_lo >= rows * n).  The split conversion honours the
 *     format's contract (csrc/device_math.h): |x| > 65504 saturates and raises the sticky range flag (advh_split_overflow),
 *     NaN stays NaN planes and leaves it clear.  Serves every Layer* class (captum.attr.LayerIntegratedGradients' path points).
 * advh_layer_tap : out[r] = g[r] * inv_scale (act == NULL: the layer gradient dF/dh_l, g the residual-stream gradient and
 *     inv_scale = 1 / loss_scale) or g[r] * inv_scale * act[r] (captum.attr.LayerGradientXActivation); row_sum != NULL also
 *     writes row_sum[r] = sum_j of those values (per-clip sums for deltas with rows = clips, per-frame relevance with
 *     rows = clips * T).  out may be NULL when row_sum is given.
 * advh_layer_conductance_accumulate (captum.attr.LayerConductance): one step-major chunk of `steps` consecutive path points,
 *     act [steps][B][n] = h_l of each point and grad [ngrad][B][n] = dF/dh_l of the first ngrad of them (the last point of the
 *     path needs no gradient; grad may be NULL when ngrad = 0).  Element (b, j) walks the points k in order:
 *     total[b] += pg * (act[k][b] - pa) (skipped for the path's first point: first = 1 and k = 0), then pa = act[k][b] and, for
 *     k < ngrad, pg = grad[k][b]; (pg, pa) start from and end in prev_grad / prev_act [B][n], which carry the pair that straddles
 *     a chunk boundary (not read when first = 1).  Over the whole path: total[b] = sum_k grad[k][b] * (act[k+1][b] - act[k][b]).
 * The activation-space path points of LayerIntegratedGradients and the weighted gradient sums of it and of
 * captum.attr.InternalInfluence are advh_attr_path_points / advh_attr_path_accumulate with n = T * H.
 * NaN / inf propagate into the results (the caller's finiteness check reports them).  Null pointers (op, act of the tap, out or
 * row_sum -- not both -- and grad with ngrad = 0 excepted), rows, B, n or steps <= 0, ngrad outside [0, steps], a flag outside
 * {0, 1}, a non-finite inv_scale and, in split mode, a plane pitch of 0 or below rows * n return ADVH_EINVAL before any HIP call. */
int advh_layer_inject(const float* src, int rows, int64_t n, float* resid, void* op, int split, int64_t op_lo, advh_stream_t stream);
int advh_layer_tap(const float* g, const float* act, float inv_scale, int rows, int64_t n, float* out, float* row_sum,
                   advh_stream_t stream);
int advh_layer_conductance_accumulate(const float* grad, const float* act, int B, int64_t n, int steps, int ngrad, int first,
                                      float* prev_grad, float* prev_act, float* total, advh_stream_t stream);

/* Neuron attributions (csrc/attribution_neuron.hip): Captum's NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap,
 * NeuronConductance and NeuronFeatureAblation of one unit, or one band of units, of hidden_states[l], restated (captum is
 * absent).  The forward stops at the layer (EmbedderGrad.forward(to_layer=l)) and the backward starts there from a seed gradient
 * (EmbedderGrad.backward(from_layer=l, ...)) and runs the lower chain down to the waveform; these kernels are the two ends.
 * A selection box is six ints (t0, t1, tstep, h0, h1, hstep) over the [T][H] frame of a clip: the normalised form of Captum's
 * neuron_selector, a pair of ints or slices -- half-open, steps > 0, an int i is (i, i + 1, 1); the neuron's value is the sum
 * over the box (Captum aggregates slices by sum).  All rows fp32, contiguous, [R][T][H] with R clip rows.  One thread per
 * element, every product rounded on its own, the box sum a fixed-shape tree in one workgroup per clip row, no atomics: equal
 * inputs give equal bits.
 *
 * advh_layer_seed : the gradient at hidden_states[l] the lower chain starts from, in place of the autograd seed of
 *     captum.attr.NeuronGradient (torch.autograd.grad of the selected neuron): resid [R * T][H] fp32, the residual-stream
 *     gradient, and, if op != NULL, its GEMM-operand copy -- one fp16 plane (split = 0) or the split format's hi plane at op and
 *     lo plane op_lo elements behind (split = 1; op_lo >= R * T * H), converted as by advh_layer_inject: |x| > 65504 saturates
 *     and raises the sticky range flag (advh_split_overflow), NaN stays NaN planes and leaves it clear.  Every element of both
 *     outputs is written, so neither needs clearing first.  Box mode (src == NULL): scale * (row_scale ? row_scale[r] : 1) inside
 *     the box of clip row r, 0 elsewhere (row_scale [R]: captum.attr.NeuronConductance's layer-gradient entry per path point).
 *     Dense mode (src [R][T][H] != NULL; box is not read, row_scale must be NULL): scale * src, any vector-Jacobian seed.
 * advh_neuron_values : out[r] = sum over the box of v[r][t][h], v [R][T][H]: the neuron's activation (the forward_func output
 *     captum.attr.NeuronFeatureAblation differences, and the s_n of the completeness checks) when v is hidden_states[l], the
 *     neuron's entry of a layer gradient (captum.attr.NeuronConductance) when v is dF/dh_l.
 * NaN / inf in the inputs propagate into the results (the caller's finiteness check reports them).  Null pointers (op, row_scale
 * and src excepted, and box in dense mode), R, T or H <= 0, an empty or out-of-range box or a step <= 0, row_scale given in dense
 * mode, a non-finite scale, a split flag outside {0, 1} and, in split mode, a plane pitch of 0 or below R * T * H return
 * ADVH_EINVAL before any HIP call. */
int advh_layer_seed(const float* src, const float* row_scale, float scale, int R, int T, int H, const int* box, float* resid, void* op,
                    int split, int64_t op_lo, advh_stream_t stream);
int advh_neuron_values(const float* v, int R, int T, int H, const int* box, float* out, advh_stream_t stream);

/* Attribution metrics (csrc/attribution_metrics.hip): Captum's infidelity and sensitivity_max of the [B][n] inputs x, restated
 * (captum is absent).  S perturbed samples per clip, processed in chunks of p consecutive samples [s0, s0 + p); a chunk's rows
 * are clip-major, row b * p + s' (Captum's repeat_interleave), and the noise of a row comes from its global counter
 * g = b * S + s0 + s' (the Philox words of advh_philox_normal), so a sample's row does not depend on the chunking.
 *
 * advh_metric_rows : rows [row0, row0 + rows) of the chunk (rr = row0 + r, clip b = rr / p) into out [rows][n], with w_k the
 *     Philox words of counter (j / 4, g) and u = (2 * (w >> 9) + 1) * 2^-24:
 *   mode 0 (sensitivity_max's default perturbation): out = x[b] + scale * (2u - 1)   (2u - 1 exact; dot must be NULL, mul 0)
 *   mode 1 (infidelity's noisy perturbation):        out = x[b] - scale * N(seed, g, :)  and
 *     dot[rr] = sum_j pert_j * attr[b][j], pert = scale * N (mul = 0) or the decorator's safe_div(x - out, x - base) (mul = 1,
 *     base[b or 0], or x itself when base is NULL; a zero denominator divides by 1).  The perturbation is never stored.
 *   Every product is rounded before its add or subtraction (no FMA contraction).
 * advh_metric_row_dot : dot[r] = sum_j pert[r][j] * attr[r / p][j], r < B * p: mode 1's dot for an explicit perturbation (a
 *     Python perturb_func), over the same fixed tree, so equal terms give equal bits.
 * advh_infidelity_fold : one thread per clip, samples in increasing order: a = dot[b * p + s], d = f0[b] - fk[b * p + s] (fp32
 *     logits F(x) [B] and F(x~) [B * p]); fp64 acc[b] += (a - d)^2, or (normalize) acc[3b .. 3b + 2] += (a^2, a d, d^2).
 *     acc starts at zero before the first chunk.
 * advh_infidelity_finalize : out[b] = acc[b] / S, or (normalize) beta = AD / (A != 0 ? A : 1) and
 *     ((beta^2 A - 2 beta AD) + D) / S, each operation in fp64, one rounding to fp32.
 * advh_row_norm : out[r] = ||v[r]||_ord over the row's fixed tree (fp32), ord 0: 2-norm, 1: 1-norm, 2: max norm.
 * advh_sensitivity_fold : ratio[b * p + s] = ||e[b] - et[b * p + s]||_ord / (enorm[b] != 0 ? enorm[b] : 1), then
 *     smax[b] = max(smax[b], ratio[...]) over s in increasing order (smax starts at zero; NaN propagates).
 * Every row reduction is one workgroup, a fixed-shape tree, no atomics.  NaN / inf propagate into the results (the caller's
 * finiteness check reports them).  Null pointers, non-positive sizes, rows outside the chunk, a scale that is negative, NaN or
 * infinite, and a mode, ord or flag out of range return ADVH_EINVAL before any HIP call.
 * Replaces captum.metrics.infidelity(...) and captum.metrics.sensitivity_max(...). */
typedef struct advh_metric_desc {
    const float* x;        /* [B][n] inputs                                                      */
    const float* attr;     /* [B][n] attributions (mode 1)                                       */
    const float* base;     /* [base_rows][n] baselines of mode 1's denominator, or NULL           */
    int64_t n;
    uint64_t seed;
    int B, S, s0, p;       /* the chunk: samples [s0, s0 + p) of each clip, s0 + p <= S            */
    int base_rows;         /* 1 or B                                                             */
    int mode;              /* 0: uniform rows (sensitivity_max), 1: Gaussian rows + dot (infidelity) */
    int mul;               /* mode 1: multiply_by_inputs                                         */
    float scale;           /* mode 0: perturb_radius, mode 1: stdevs                             */
} advh_metric_desc;
int advh_metric_rows(const advh_metric_desc* d, int64_t row0, int rows, float* out, float* dot, advh_stream_t stream);
int advh_metric_row_dot(const float* pert, const float* attr, int B, int p, int64_t n, float* dot, advh_stream_t stream);
int advh_infidelity_fold(const float* dot, const float* f0, const float* fk, int B, int p, int normalize, double* acc, advh_stream_t stream);
int advh_infidelity_finalize(const double* acc, int B, int S, int normalize, float* out, advh_stream_t stream);
int advh_row_norm(const float* v, int rows, int64_t n, int ord, float* out, advh_stream_t stream);
int advh_sensitivity_fold(const float* e, const float* et, const float* enorm, int B, int p, int64_t n, int ord, float* ratio,
                          float* smax, advh_stream_t stream);

/* Adversarial attacks (csrc/attribution_robust.hip): Captum's FGSM and PGD (captum.robust) on the [B][n] clips, restated from
 * Captum 0.7's robust/_core/fgsm.py and pgd.py (captum is absent).  These kernels are the iterate update between two
 * forward + backward pairs of the gradient chain; all rows fp32, contiguous.  Every product, sum and difference is rounded on
 * its own (no FMA contraction), as the unfused torch expressions round them.
 *
 * advh_robust_step : launch rows [row0, row0 + rows) of the B * p rows into out [rows][n]; row r is clip b = r / p and ladder
 *     index k = r % p (p = 1 for FGSM and PGD proper; p = K builds an epsilon ladder).  x and grad have B rows (indexed by b) or
 *     B * p rows (indexed by r).  Per element j:
 *       gl = seed[b] * grad[.][j]                       seed = dL/d logit per clip, NULL = 1: the chain runs with the unit seed
 *                                                       and the per-clip factor is applied here (the loss gradient, by linearity)
 *       e  = (float)(multiplier * eps[k])               multiplier = -1 if targeted else +1, the product in double (a Python float)
 *       v  = |gl| > 1e-6f ? x + (e * sign(gl)) * mask : x
 *            -- FGSM._perturb: torch.where(torch.abs(grad) > self.zero_thresh, inp + multiplier * epsilon * torch.sign(grad) * mask,
 *            inp); zero_thresh = 10 ** -6 is a constant here; mask NULL gives x + e * sign(gl); mask is [1][n] or [B][n]
 *       norm 0 : no projection (FGSM)
 *       norm 1 : v = x0 + clamp(v - x0, -radius, radius)          -- PGD._clip, "Linf": inputs + torch.clamp(diff, -radius, radius)
 *       norm 2 : d = v - x0, s = sqrt(sum_j d^2), v = x0 + d * (s > radius ? radius / (s + 1e-7f) : 1)
 *            -- PGD._clip, "L2": inputs + torch.renorm(diff, 2, 0, radius); the row sum is a fixed-shape tree in one workgroup
 *            (thread t adds quads t, t + 256, ... in order, then a wave64 xor tree and (w0 + w1) + (w2 + w3)); the second pass
 *            recomputes d, so the row is never staged
 *       out = clamp(v, lo, hi)                          -- self.bound: torch.clamp(x, min=lower_bound, max=upper_bound); -+inf allowed
 *     out may alias the launch rows of x.  eps is a HOST array of p doubles (p <= ADVH_ROBUST_MAX_P): the p step sizes travel as
 *     kernel arguments.
 * advh_robust_random_start : PGD._random_point, bounded; clip b draws from Philox row b of seed (the words of advh_philox_normal):
 *       norm 1 : out = clamp(x0 + radius * (2u - 1), lo, hi), u the uniforms of advh_metric_rows' mode 0 (the row of S = 1, p = 1)
 *            -- torch.rand_like(center) * radius * 2 - radius
 *       norm 2 : out = clamp(x0 + (r_b / ||z||) * z, lo, hi), z = N(seed, b, :), ||z|| over the same tree, r_b = radius * u_b^(1/n),
 *            u_b the first uniform of Philox row B + b  -- F.normalize(torch.randn_like(center)) * torch.rand(B) ** (1 / d) * radius
 * advh_robust_first_flip : the fold of an epsilon ladder, one thread per clip, k in increasing order: out[b] = eps[k] (a device
 *     array of K floats) and first[b] = k of the first k with (logit[b * K + k] > 0) != (clean_logit[b] > 0); +inf and K when no
 *     k flips the decision.
 * No atomics: equal inputs give equal bits, for every split of the rows over launches.  NaN / inf propagate into the results
 * (the caller's finiteness check reports them).  Null pointers (seed and mask excepted, and x0 when norm == 0), non-positive
 * sizes, p above ADVH_ROBUST_MAX_P, an unknown norm, a targeted flag outside {0, 1}, a radius or eps that is negative or not
 * finite, lo > hi or a NaN bound, x_rows / grad_rows that are neither B nor B * p, mask_rows neither 1 nor B, a row window outside
 * B * p and B * p (B * K) above int range return ADVH_EINVAL before any HIP call.
 * Replaces captum.robust.FGSM(...).perturb(...) and captum.robust.PGD(...).perturb(...). */
#define ADVH_ROBUST_MAX_P 64
typedef struct advh_robust_desc {
    const float* x0;       /* [B][n] clean clips: the projection's centre (norm 1, 2)            */
    const float* x;        /* [x_rows][n] current iterate                                       */
    const float* grad;     /* [grad_rows][n] d logit / d x of the unit seed                     */
    const float* seed;     /* [B] dL/d logit per clip, or NULL (1)                              */
    const float* mask;     /* [mask_rows][n], or NULL                                           */
    const double* eps;     /* HOST [p] step sizes, each finite and >= 0                         */
    int64_t n;
    int B, p;
    int x_rows, grad_rows; /* B or B * p                                                        */
    int mask_rows;         /* 1 or B                                                            */
    int targeted;          /* 0: multiplier +1, 1: multiplier -1                                */
    int norm;              /* 0: none (FGSM), 1: Linf, 2: L2                                    */
    float radius;          /* norm 1, 2: finite, >= 0                                           */
    float lo, hi;          /* the bounds, lo <= hi, -+inf allowed                               */
} advh_robust_desc;
int advh_robust_step(const advh_robust_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_robust_random_start(const float* x0, int B, int64_t n, uint64_t seed, int norm, float radius, float lo, float hi, float* out,
                             advh_stream_t stream);
int advh_robust_first_flip(const float* logit, const float* clean_logit, const float* eps, int B, int K, float* out, int* first,
                           advh_stream_t stream);

/* Perturbation attributions (csrc/attribution_ablation.hip): Captum's Occlusion and FeatureAblation of the [B][n] inputs x,
 * restated (captum is absent).  K perturbations; the ablated rows are perturbation-major, row g = k * B + b (Captum's
 * input.repeat), and F is the classifier logit.
 *   mode 0 (Occlusion, window win, stride): K = ceil((n - win) / stride) + 1; window k covers [k * stride, min(k * stride + win,
 *     n)) (Captum pads the window with a negative right pad, which crops the last one).  Captum asserts win <= n and
 *     stride <= win unless win == n.
 *   mode 1 (FeatureAblation): mask[.][t] in [0, K) is the feature index of sample t; ablation k replaces every sample of
 *     feature k in every clip at once.
 * Ablated row (k, b): base[b or 0][t] where sample t is in window / feature k, x[b][t] elsewhere (Captum's
 * x * (1 - m) + base * m).  diff[k][b] = F(x)[b] - F(ablated)[k * B + b], fp32.
 *   Occlusion:       attr[b][t] = (sum_{k = k_lo..k_hi} diff[k][b], in increasing k) / (k_hi - k_lo + 1), with
 *                    k_lo = max(0, ceil((t - win + 1) / stride)), k_hi = min(K - 1, t / stride) -- Captum's
 *                    total_attrib += diff * mask; weights += mask; total_attrib / weights, bit for bit for finite diffs.
 *   FeatureAblation: attr[b][t] = diff[mask[t]][b] (a mask entry outside [0, K) yields NaN).
 *
 * advh_ablation_points     : out[r] = ablated row g = row0 + r ([rows][n]); rows g >= K * B copy x[g % B] (padding of a
 *                            fixed-shape last chunk).  rows = 0 launches nothing.
 * advh_ablation_accumulate : attr [B][n] from f0 = F(x) [B] and fk = F(ablated) [K * B]; one launch, one thread per (b, t),
 *                            no atomics.
 * Replaces captum.attr.Occlusion / captum.attr.FeatureAblation(model).attribute(x, ...) on the waveform -> logit classifier. */
typedef struct advh_ablation_desc {
    const float* x;        /* [B][n] inputs                                                     */
    const float* base;     /* [base_rows][n] baselines, base_rows = 1 or B                       */
    const int32_t* mask;   /* [mask_rows][n] feature index, mask_rows = 1 or B (mode 1; ignored in mode 0) */
    int64_t n;
    int B, base_rows, mask_rows;
    int mode;              /* 0: Occlusion, 1: FeatureAblation                                   */
    int win, stride;       /* mode 0 only                                                        */
    int K;                 /* perturbations (mode 0: must equal the formula above)               */
} advh_ablation_desc;
int advh_ablation_points(const advh_ablation_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_ablation_accumulate(const advh_ablation_desc* d, const float* f0, const float* fk, float* attr, advh_stream_t stream);

/* Captum's Occlusion for a 2-D input (csrc/attribution_spectral.hip): x [B][Fm][Tm] (the STFT mask), windows (wf, wt) every
 * (sf, st), cropped at the edges.  Per axis K = ceil((n - w) / s) + 1 (w <= n, and s <= w unless w == n); window
 * k = kf * Kt + kt, first dimension slowest, as Captum's _occlusion_mask enumerates; occluded rows are k * B + b.
 *   advh_occlusion2d_points     : out[r] = occluded row g = row0 + r ([rows][Fm * Tm]); rows g >= Kf * Kt * B copy x[g % B].
 *   advh_occlusion2d_accumulate : attr[b][f][t] = (sum of f0[b] - fk[k * B + b] over the windows k covering (f, t), in
 *                                 increasing k) / their count; one thread per bin, no atomics.                        */
typedef struct advh_occlusion2d_desc {
    const float* x;        /* [B][Fm * Tm] inputs                                               */
    const float* base;     /* [base_rows][Fm * Tm] baselines, base_rows = 1 or B                 */
    int B, base_rows;
    int Fm, Tm;
    int wf, wt, sf, st;    /* window and stride per axis                                        */
    int Kf, Kt;            /* windows per axis (must equal the formula above)                    */
} advh_occlusion2d_desc;
int advh_occlusion2d_points(const advh_occlusion2d_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_occlusion2d_accumulate(const advh_occlusion2d_desc* d, const float* f0, const float* fk, float* attr, advh_stream_t stream);

/* Band x segment relevance: out [B][nb][ns] = sums of attr [B][Fm][Tm] over boxes of bw bins x sw frames, nb = ceil(Fm / bw),
 * ns = ceil(Tm / sw), the last box of an axis cropped.  One workgroup and one fixed-shape tree per box, no atomics. */
int advh_tf_pool(const float* attr, int B, int Fm, int Tm, int bw, int sw, float* out, advh_stream_t stream);

/* Shapley attributions over feature groups (csrc/attribution_shapley.hip): Captum's ShapleyValueSampling, ShapleyValues and
 * KernelShap of the [B][n] inputs x, restated (captum is absent).  index[.][t] in [0, K) is the feature of sample t (the rank of
 * its id among the ids present); F is the classifier logit.  A coalition row keeps x[b][t] where the feature of t is in the
 * coalition and base[b or 0][t] elsewhere (Captum's baseline * (1 - m) + x * m).
 *   mode 0 (rank; ShapleyValueSampling over P drawn permutations, ShapleyValues over all K! in itertools order): rank[pl][k] is
 *     the position of feature k in permutation p = p0 + pl of the table.  Row g = (p * K + j) * B + b keeps the features of
 *     rank <= j: step j switches feature perm_p[j] from the baseline to x in every clip at once.
 *       diff[p][j][b] = F(row p, j, b) - F(row p, j - 1, b), F(row p, -1, b) = F(base)[b];
 *       attr[b][t] = (sum_p diff[p][rank_p(index[b][t])][b], in increasing p from 0.f) / P -- Captum's
 *       total_attrib += eval_diff * mask; total_attrib / iter_count, bit for bit for finite logits.
 *   mode 1 (presence; KernelShap): present[g][k] != 0 when row g keeps feature k.  The host fits each clip's weighted linear
 *     regression on the logits and scatters its coefficients: attr[b][t] = coef[b][index[b][t]].
 * A feature index outside [0, K) yields NaN (a rank outside [0, K) too, in the accumulation).
 *
 * advh_coalition_points   : out[r] = coalition row g = row0 + r ([rows][n]); rows past the table (rank mode: g >= (p0 + P) * K * B,
 *                           presence mode: g >= rows) copy x[g % B] (padding of a fixed-shape last chunk).  Rank mode needs
 *                           row0 >= p0 * K * B.  rows = 0 launches nothing.
 * advh_shapley_accumulate : total [B][n] += the diffs of permutations [p0, p0 + np) (inside the table), fk = F(rows of those
 *                           permutations) [np * K * B] starting at permutation p0, fbase = F(base) [B]; finalize_div > 0 then
 *                           divides once (__fdiv_rn), 0 leaves the sum.  Rank mode only; x, base ignored.  One launch, one
 *                           thread per (b, t), no atomics.
 * advh_coalition_scatter  : attr [B][n] = coef [B][K] gathered through the index map; x, base and the tables ignored.
 * Replaces captum.attr.ShapleyValueSampling / ShapleyValues / KernelShap(model).attribute(x, ...) on the waveform -> logit
 * classifier. */
typedef struct advh_coalition_desc {
    const float* x;          /* [B][n] inputs                                                   */
    const float* base;       /* [base_rows][n] baselines, base_rows = 1 or B                     */
    const int32_t* index;    /* [index_rows][n] feature index, index_rows = 1 or B               */
    const int32_t* rank;     /* mode 0: [P][K] rank of each feature in each permutation          */
    const uint8_t* present;  /* mode 1: [rows][K] coalition membership of each row               */
    int64_t n;
    int64_t p0;              /* mode 0: the permutation the table starts at                      */
    int64_t rows;            /* mode 1: rows of the table                                        */
    int B, base_rows, index_rows;
    int mode;                /* 0: rank (Shapley), 1: presence (KernelShap)                      */
    int K;                   /* features (row length of the tables)                              */
    int P;                   /* mode 0: permutations in the table                                */
} advh_coalition_desc;
int advh_coalition_points(const advh_coalition_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_shapley_accumulate(const advh_coalition_desc* d, const float* fbase, const float* fk, int64_t p0, int np, float* total,
                            float finalize_div, advh_stream_t stream);
int advh_coalition_scatter(const advh_coalition_desc* d, const float* coef, float* attr, advh_stream_t stream);

/* Lime and FeaturePermutation (csrc/attribution_lime.hip): Captum's Lime and FeaturePermutation of the [B][n] inputs x,
 * restated (captum is absent).
 *   FeaturePermutation: index[t] in [0, K) is the feature of sample t (one mask for every clip, Captum's assert); perm[k][b] is
 *     the clip whose samples row (k, b) takes on feature k, a permutation of [0, B) that is not the identity, drawn per feature
 *     on the host.  Rows are perturbation-major, row g = k * B + b (FeatureAblation's order):
 *       row (k, b)[t] = x[perm[k][b]][t] where index[t] == k, x[b][t] elsewhere (Captum's _permute_feature).
 *     attr[b][t] = F(x)[b] - F(row index[t], b) is advh_ablation_accumulate in mode 1 with mask = index (base unread).
 *   Lime: the perturbed rows are KernelShap's presence-mode coalition rows (advh_coalition_points, mode 1: row s * B + b keeps
 *     x[b] on the features drawn on and the baseline elsewhere), and the weight of row g against its clip x[g % B] is Captum's
 *     get_exp_kernel_similarity_function(mode, w): exp(-d^2 / (2 w^2)), d computed on the raw row the classifier reads:
 *       mode 0 (cosine):    d = 1 - <x, v> / (max(||x||, 1e-8) * max(||v||, 1e-8))   (torch.nn.CosineSimilarity(dim=0))
 *       mode 1 (euclidean): d = ||x - v||
 *     The host fits each clip's interpretable model on (draws, logits, weights); the default SkLearnLasso solves with
 *     advh_lasso_cd, and the coefficients go back to the samples with advh_coalition_scatter.
 *
 * advh_permutation_points : out[r] = permuted row g = row0 + r ([rows][n]); rows g >= K * B copy x[g % B] (padding of a
 *                           fixed-shape last chunk).  A perm entry outside [0, B) gives NaN on that feature's samples; an index
 *                           outside [0, K) keeps x.  Needs B >= 2.  rows = 0 launches nothing.
 * advh_row_similarity     : sim[row0 + r] for the chunk rows [rows][n] (row r is global row g = row0 + r, clip g % B), one
 *                           workgroup per row: the sums (<x, v>, ||x||^2, ||v||^2, or ||x - v||^2) in fp64 over a fixed order
 *                           (so a row's weight does not depend on the chunking), exp in fp64, one rounding to fp32.  It only
 *                           reads the chunk, so it may run before or after the forward that reads the same rows.  rows = 0
 *                           launches nothing.
 * advh_lasso_cd           : HOST function, no HIP call.  Minimises 1/2 ||y - X c||^2 + alpha ||c||_1 (X [S][K] given column
 *                           by column: column k at X + k * S; the caller centres and scales by sqrt(w / sum w), which makes it
 *                           sklearn's weighted Lasso) by cyclic coordinate descent from the coef passed in, in fp64.  The
 *                           duality gap (sklearn's, on a residual recomputed from scratch) is evaluated when the largest step of
 *                           a sweep is <= tol relative to the largest coefficient, and after sweep max_iter; the solve stops at
 *                           gap <= tol * ||y||^2.  Writes the last gap and the sweeps done (== max_iter with gap > tol ||y||^2:
 *                           not converged).
 * Null pointers, non-positive sizes, B < 2 (permutation), a mode outside [0, 1], a kernel width that is not finite and > 0, a
 * negative or non-finite alpha or tol, and max_iter < 1 return ADVH_EINVAL before any HIP call.
 * Replaces captum.attr.Lime(model).attribute(x, ...) and captum.attr.FeaturePermutation(model).attribute(x, ...) on the
 * waveform -> logit classifier. */
typedef struct advh_permutation_desc {
    const float* x;          /* [B][n] inputs                                                   */
    const int32_t* index;    /* [n] feature index of each sample                                */
    const int32_t* perm;     /* [K][B] source clip of row (k, b)                                */
    int64_t n;
    int B, K;
} advh_permutation_desc;
int advh_permutation_points(const advh_permutation_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_row_similarity(const float* rows_ptr, const float* x, int64_t row0, int rows, int B, int64_t n, int mode, float kernel_width,
                        float* sim, advh_stream_t stream);
int advh_lasso_cd(const double* X, const double* y, int S, int K, double alpha, double tol, int max_iter, double* coef, double* gap,
                  int* iters);

/* Perturbation curves of an attribution map (csrc/attribution_curve.hip): the deletion / insertion curves of Petsiuk et al.
 * (RISE, BMVC 2018, sec. 4.1) and the AOPC of Samek et al. (2017) in MoRF / LeRF order -- DeYoung et al.'s (2020)
 * comprehensiveness / sufficiency -- restated from the papers (no Captum class exists).  Rows are [B][n] fp32; index[1 | B][n] in
 * [0, K) is the feature of sample t; index == NULL is the identity (K == n, every sample its own feature).  All four entry points
 * are deterministic: no atomics, a fixed order, bit-identical results from run to run.
 *
 * advh_feature_scores : score[b][k] = the fp32 sum, IN INCREASING t from 0.f, of attr[b][t] (use_abs: |attr[b][t]|) over the
 *                       samples of feature k; mean != 0 divides once by the sample count (__fdiv_rn).  The order is the
 *                       contract: a sequential fp32 replay on the host gives the same bits (so a lone -0 scores +0).  A feature
 *                       with no sample in clip b scores -inf (last in MoRF, first in LeRF; the Python engine refuses such a
 *                       mask).  Samples whose index is outside [0, K) belong to no feature.
 * advh_feature_rank   : rank[b][k] (int32) = the number of features j of clip b that come before k.  descending != 0 (MoRF):
 *                       j comes before k when s_j > s_k, or s_j == s_k && j < k; otherwise (LeRF): when s_j < s_k, or
 *                       s_j == s_k && j < k.  -0 == +0, +-inf order as numbers; NaN scores are the caller's to refuse (they
 *                       order as their bit patterns; the result is still a permutation).  Exact: every row of rank is a
 *                       permutation of [0, K), any K >= 1.  K * K key comparisons per clip (counting rank over LDS tiles).
 * advh_curve_points   : out[r] = curve row g = row0 + r ([rows][n]), step j = g / B of clip b = g % B (perturbation-major, as
 *                       the ablation rows).  Sample t is switched when rank[b][index[t]] < counts[j].  mode 0 (deletion): a
 *                       switched sample takes base[b or 0][t], the rest x[b][t]; mode 1 (insertion): a switched sample takes x,
 *                       the rest base.  A feature index outside [0, K) writes NaN into that sample.  Rows g >= S1 * B copy
 *                       x[g % B] (padding of a fixed-shape last chunk).  rows = 0 launches nothing.
 * advh_curve_fold     : from fk [S1 * B] (the rows' fp32 logits), one thread per clip, steps in increasing j:
 *                       y_j = fk[j * B + b], or 1 / (1 + expf(-fk)) with prob != 0; curve[b][j] = y_j; with f_j = counts[j] / K
 *                       in fp64, accumulated in fp64 and rounded once to fp32:
 *                         auc[b]  = sum_j (f_{j+1} - f_j) (y_j + y_{j+1}) / 2 / (f_last - f_0)
 *                         aopc[b] = (1 / (S1 - 1)) sum_{j != ref} (y_ref - y_j),  ref = 0, or S1 - 1 with ref_last != 0
 *                       (the row that equals x: step 0 of a deletion, the last step of an insertion).  S1 >= 2.
 * counts [S1] int32 lives on the DEVICE: c_0 < c_1 < ... < c_{S1-1} inside [0, K].  Null pointers, non-positive sizes, K > n,
 * B > 65535 (scores, rank), index_rows / base_rows not in {1, B}, index == NULL with K != n, a mode outside [0, 1] and an S1 that
 * no strictly increasing counts inside [0, K] can have (S1 > K + 1; fold: S1 < 2) return ADVH_EINVAL before any HIP call.  The
 * values of counts cannot be read before a HIP call: advh_curve_fold checks them on the device and writes NaN into auc and
 * aopc when they are not strictly increasing inside [0, K]; the Python engine builds them on the host and refuses bad ones. */
typedef struct advh_curve_desc {
    const float* x;          /* [B][n] inputs                                                   */
    const float* base;       /* [base_rows][n] baselines, base_rows = 1 or B                     */
    const int32_t* index;    /* [index_rows][n] feature index, index_rows = 1 or B; NULL: identity */
    const int32_t* rank;     /* [B][K] rank of each feature in each clip's order                 */
    const int32_t* counts;   /* [S1] features switched at each step (device memory)              */
    int64_t n;
    int B, base_rows, index_rows;
    int K;                   /* features                                                         */
    int S1;                  /* steps of the curve (S + 1)                                       */
    int mode;                /* 0: deletion, 1: insertion                                        */
} advh_curve_desc;
int advh_feature_scores(const float* attr, const int32_t* index, int index_rows, int B, int64_t n, int K, int use_abs, int mean,
                        float* score, advh_stream_t stream);
int advh_feature_rank(const float* score, int B, int K, int descending, int32_t* rank, advh_stream_t stream);
int advh_curve_points(const advh_curve_desc* d, int64_t row0, int rows, float* out, advh_stream_t stream);
int advh_curve_fold(const float* fk, const int32_t* counts, int B, int S1, int K, int prob, int ref_last, float* curve, float* auc,
                    float* aopc, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * fp32-class ("split") mode.  The reference computes the whole path in fp32 (addvisor.py:12-84,
 * transformers/models/wav2vec2/modeling_wav2vec2.py:254-802 under audioprocessor.py:69-77).  In this mode every tensor
 * that the fp16 path stores as fp16 is a PAIR of fp16 planes (hi, lo) with x = hi + lo * 2^-11 (hi = fp16(x),
 * lo = fp16((x - hi) * 2^11); csrc/device_math.h) -- ~22 significand bits -- and every matrix product runs as three fp16
 * MFMAs with fp32 accumulation (advh_gemm_desc.split).  The entry points below are the split-format variants of the row /
 * direct kernels above: same arithmetic, `*_lo` = distance in ELEMENTS from a tensor's hi plane to its lo plane (both planes
 * share one addressing).  fp32 tensors (residual stream, masks, waveforms, statistics) are unchanged.                     */
/* RANGE of the split format: hi is an fp16, so a value must satisfy |x| <= 65504 (the reference's fp32: 3.4e38).  Every kernel
 * that WRITES a split tensor saturates a larger value, +-inf included (hi = +-65504, lo = the clamped remainder: +-65535.98 in
 * all), instead of producing inf / NaN planes, and raises a sticky process-wide flag in host-mapped memory.  A NaN is written
 * as NaN planes (hi = lo = NaN) and does NOT raise the flag, also where it shares a conversion vector with an out-of-range
 * value; in range (|x| <= 65504) the planes keep x to ~2^-22 relative (|x| < 2^-14: hi = 0, x carried by lo alone).  Every
 * producer is held to this in tests/test_gpu_split_contract.py.  advh_split_overflow returns the flag (1 = some kernel that
 * has already run met an out-of-range value since the last reset) and clears it when reset != 0; it reads
 * host memory only -- no synchronisation -- so a kernel still in flight is seen by a later call.  Weights are range-checked
 * on the host when they are packed.                                                                                     */
int advh_split_overflow(int reset);
int advh_w2v2_frontend_split(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                             const float* bias0, const float* gamma, const float* beta, int mode, int normalize, float* stats_ws,
                             float* norm_ws, float* mr_ws, void* out, int64_t out_lo, int T0, int P0, int C0, advh_stream_t stream);
/* in: fp32 rows (in_is_f32, in_lo ignored) or a split pair; add_h: NULL or a split pair; out_h: NULL or a split pair. */
int advh_layernorm_split(const void* in, int in_is_f32, int64_t in_ld, int64_t in_lo, const void* add_h, int64_t add_ld,
                         int64_t add_lo, const float* gamma, const float* beta, float* out_f, void* out_h, int64_t out_ld,
                         int64_t out_lo, int M, int C, float eps, int gelu, advh_stream_t stream);
int advh_posconv_gather_split(const float* h, void* xg, int64_t xg_lo, int B, int T, int H, int G, int K, int pad_left,
                              advh_stream_t stream);
/* softmax(Q K^T / sqrt(d)) V on split q | k | v -> split ctx; T <= 256, head dim a multiple of 8 up to 128 (above 64 the keys
 * stream through LDS in blocks with an online softmax: XLS-R's head dim 120). */
int advh_attention_split(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, int B, int T, int H, int heads,
                         advh_stream_t stream);
int advh_unet_stem_split(const float* mag, int Fq, int Tq, int B, int H, int W, const float* wgt, const float* bias,
                         void* out, int64_t out_lo, int PH, int PW, float slope, advh_stream_t stream);
int advh_unet_pack_x_split(const float* mag, int Fq, int Tq, int B, int H, int W, void* cat, int64_t cat_lo, int C, int c0,
                           int PH, int PW, advh_stream_t stream);
int advh_unet_head_split(const void* y, int64_t y_lo, int B, int H, int W, int PH, int PW, const float* wgt, float bias,
                         float* mask, float* logits, advh_stream_t stream);
/* fp32-class input-gradient chain (captum_saliency.py:116-135: fp32 autograd through the embedder; loss_function.py:46-53 +
 * train_addvisor.py:376: loss.backward() through the frozen embedder).  Dense dgrad products are advh_gemm_f16 launches with
 * desc.split = 1 (transposed split weights, split gradients; dact_src / out_pre are plane pairs sharing o_lo); these are the
 * split-format forms of the row kernels above -- same arithmetic, fp16 tensors replaced by plane pairs -- and the attention
 * backward (head dim a multiple of 8 up to 128, T <= 256): head dims <= 64 in split arithmetic (three fp16 MFMAs per product,
 * csrc/attention_bwd_x3.hip), larger ones on the fp32-input matrix instruction v_mfma_f32_16x16x4_f32 (csrc/attention_bwd_f32.hip;
 * advh_set_option("attention_bwd_mfma_f32", 1) selects it for every head dim).  */
int advh_layernorm_bwd_split(const void* x, int x_is_f32, int64_t x_lo, const void* dy, int dy_is_f32, int64_t dy_lo,
                             const float* gamma, const float* beta, int gelu_fwd, const float* add, const void* dact_src,
                             int64_t dact_lo, float* out_f, void* out_h, int64_t out_lo, int M, int C, float eps, int remap_T,
                             int remap_P, advh_stream_t stream);
int advh_attention_bwd_split(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                             int B, int T, int H, int heads, advh_stream_t stream);
int advh_pool_logreg_bwd_split(const float* coef, const float* dlogit, float* dh, void* dh16, int64_t dh16_lo, int B, int T, int H,
                               advh_stream_t stream);
/* Attention maps and rollout (csrc/attention_maps.hip; Abnar & Zuidema 2020, Chefer et al. 2021 -- restated from the publications,
 * neither Captum nor the reference has them).  The attention kernels never write the T x T probabilities; this one recomputes them
 * from the saved qkv [B*T][3H] (q | k | v) of one layer, on v_mfma_f32_16x16x4_f32 for both operand formats:
 *   dctx == NULL : out = P = softmax(Q K^T / sqrt(d))            (rows are queries)
 *   dctx != NULL : out = max(P * (dO V^T * dscale), 0)           (dO = the head's slice of dctx [B*T][H]; dscale = 1 / loss_scale)
 * qkv_lo == 0: plain fp16 operands (dctx_lo must be 0 too); otherwise split plane pairs, lo planes qkv_lo / dctx_lo elements behind
 * (positive multiples of 8; dctx_lo is ignored when dctx is NULL).  fuse: 0 = none, out [B][heads][T][T]; 1 = mean, 2 = max, 3 = min
 * over heads, out [B][T][T] -- reduced inside the kernel in head order (no atomics, no per-head buffer: results are bit-identical
 * from run to run and do not depend on B).  out is fp32 and every element is written; NaN in gives NaN out, and there is no range
 * flag to raise.  T <= 256, head dim a multiple of 8 up to 128 (ADVH_EUNSUPPORTED otherwise); NULL qkv / out, B, T, heads <= 0,
 * H % heads, a fuse outside [0, 3], a bad plane distance and a non-finite dscale return ADVH_EINVAL before any HIP call.  */
int advh_attention_maps(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, float dscale, int fuse, float* out,
                        int B, int T, int H, int heads, advh_stream_t stream);
/* One rollout step on fp32 [B][T][T] matrices, row i of Y:
 *   (alpha * X[i,:] + beta * sum_k M[i,k] X[k,:] + gamma * M[i,:]) / (normalize ? alpha + beta * sum_k M[i,k] : 1)
 * plain rollout R <- rownorm(R + M R): (1, 1, 0, 1); gradient rollout on D = R - I, D <- D + A + A D: (1, 1, 1, 0).  The product runs
 * on v_mfma_f32_16x16x4_f32 with X tiled through LDS.  T <= 256 (ADVH_EUNSUPPORTED above); NULL pointers, Y == X, Y == M and
 * B, T <= 0 return ADVH_EINVAL before any HIP call.  */
int advh_rollout_step(const float* M, const float* X, float* Y, float alpha, float beta, float gamma, int normalize, int B, int T,
                      advh_stream_t stream);
/* rel [B][T]: rel[b][j] = (1/T) sum_i X[b][i][j] (the classifier mean-pools over time), rows summed in order.  Same checks.  */
int advh_rollout_relevance(const float* X, float* rel, int B, int T, advh_stream_t stream);
/* Conservative propagation through the encoder (csrc/lrp.hip; Ali et al., ICML 2022, and the GELU identity rule of AttnLRP,
 * Achtibat et al. 2024 -- restated from the publications, neither Captum nor the reference has them): gradient x input through a
 * copy of the network in which one factor of each nonlinearity is a constant of the backward pass.
 * AH-rule, ctx = sg(P) V: dqkv [B*T][3H] from the saved qkv [B*T][3H] (q | k | v) and dctx [B*T][H] of one layer, in the chain's
 * own format -- zeros in the Q and K thirds, dV[k,:] = sum_q P[q,k] dO[q,:] per (clip, head) in the V third, P = softmax(Q K^T /
 * sqrt(d)) recomputed on v_mfma_f32_16x16x4_f32 for both operand formats.  Every element of dqkv is written.  qkv_lo == 0: plain
 * fp16 (dctx_lo and dqkv_lo must be 0 too); otherwise split plane pairs, lo planes qkv_lo / dctx_lo / dqkv_lo elements behind
 * (positive multiples of 8), the V third through the checked conversion (|x| > 65 504 saturates and raises the sticky range flag, NaN
 * stays NaN planes, unflagged).  No atomics: results are bit-identical from run to run and do not depend on B.  T <= 256, head dim a
 * multiple of 8 up to 128 (ADVH_EUNSUPPORTED otherwise); NULL pointers, B, T, H, heads <= 0, H % heads and a bad plane distance
 * return ADVH_EINVAL before any HIP call.  */
int advh_attention_bwd_value(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo, int B,
                             int T, int H, int heads, advh_stream_t stream);
/* LN-rule, y = gamma (x - mean(x)) / sg(sigma) + beta: dx = u - mean_C(u) (+ add), u = gamma dy rstd, rows [M][C]; the encoder-side
 * subset of advh_layernorm_bwd(_split)'s arguments (no gelu_fwd, dact_src or remap), the same row statistics recomputed from x in
 * the same order (rstd is the same bits).  x / dy fp32 or fp16 (_split: plane pairs, x_lo / dy_lo / out_lo positive multiples of 4
 * for every fp16-side tensor), add fp32 or NULL, at least one of out_f (fp32) / out_h.  C % 4 == 0, C <= 2048 (ADVH_EUNSUPPORTED
 * above); NULL x / dy / gamma, no output, M, C <= 0 and a bad plane distance return ADVH_EINVAL before any HIP call.  */
int advh_layernorm_bwd_frozen(const void* x, int x_is_f32, const void* dy, int dy_is_f32, const float* gamma, const float* add,
                              float* out_f, void* out_h, int M, int C, float eps, advh_stream_t stream);
int advh_layernorm_bwd_frozen_split(const void* x, int x_is_f32, int64_t x_lo, const void* dy, int dy_is_f32, int64_t dy_lo,
                                    const float* gamma, const float* add, float* out_f, void* out_h, int64_t out_lo, int M, int C,
                                    float eps, advh_stream_t stream);
/* GELU identity rule, GELU(x) = x sg(Phi(x)): out[i] = d[i] * Phi(g1[i]), i < n, Phi = (1 + erf(x / sqrt 2)) / 2 from the kernels'
 * fast_erf.  d_lo == 0: fp16 (g1_lo and out_lo must be 0 too); otherwise plane pairs (lo planes >= n elements behind) joined,
 * multiplied in fp32 and re-split through the checked conversion.  out may be d.  Any n: eight elements per thread when every
 * pointer and plane distance is 16-byte aligned, the n % 8 tail (or everything) one by one.  NULL pointers, n <= 0 and a bad
 * plane distance return ADVH_EINVAL before any HIP call.  */
int advh_gelu_identity_bwd(const void* d, int64_t d_lo, const void* g1, int64_t g1_lo, void* out, int64_t out_lo, int64_t n,
                           advh_stream_t stream);
/* fp32 -> split format on the device: dst[i] = hi, dst[dst_lo + i] = lo of src[i], i < n (csrc/device_math.h split_f32: saturates
 * and raises the sticky range flag above 65 504, NaN stays NaN unflagged; any n, the n % 4 tail converted one by one).  The per-step weight refresh of the training path (train_addvisor.py:376-378
 * steps the fp32 parameters with Adam; addvisor_hip/gemm.py GemmPlan.load_weights re-packs them).  src 16-byte aligned. */
int advh_split_f32(const float* src, void* dst, int64_t dst_lo, int64_t n, advh_stream_t stream);
/* dh [B][T][H] fp32 times GELU'(dact_src) (split pre-activation of the positional conv) -> split xg, rows [pad_left, pad_left+T) */
int advh_posconv_gather_bwd_split(const float* dh, void* xg, int64_t xg_lo, int B, int T, int H, int G, int K, int pad_left,
                                  const void* dact_src, int64_t dact_lo, advh_stream_t stream);
int advh_w2v2_frontend_bwd_group_split(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                       const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                       const void* dy0, int64_t dy_lo, float* part_ws, float* sums_ws, void* dz0, int64_t dz_lo,
                                       int T0, int P0, int C0, advh_stream_t stream);
/* fp32-class form of advh_resblock_pair_f16 for the 32-channel stage (csrc/resblock_pair_x3.hip): X / out_h are split-format maps
 * [2][M][32] (lo plane x_lo / o_lo elements behind), W1 / W2 [2][k][C_out][C_in] fp16 planes (w_lo elements apart), three MFMAs
 * per product in the K order of the x3 implicit GEMM.  C = 32 only; advh_resblock_pair_x3_lds_bytes < 0: unsupported.       */
typedef struct advh_resblock_x3_desc {
    const void* X;
    const void* W1;
    const float* b1;
    const void* W2;
    const float* b2;
    void* out_h;
    int M, Wg, w0, w1, k, dil;
    float slope;
    int64_t x_lo, o_lo, w_lo;
} advh_resblock_x3_desc;
int advh_resblock_pair_x3_lds_bytes(int C, int k, int dil);
int advh_resblock_pair_x3(const advh_resblock_x3_desc* d, int C, advh_stream_t stream);
/* HiFi-GAN generator pieces on split-format maps [2][B][T+2*halo][C] (the Conv1d / ConvTranspose1d layers are advh_gemm_f16
 * launches with desc.split = 1; advh_halo_fill_f16 serves both planes when called with 2*B maps).  `pad` = inference padding. */
int advh_hifigan_pack_mel_split(const float* mel, void* out, int64_t out_lo, int B, int C, int T, int pad, int halo,
                                advh_stream_t stream);
int advh_hifigan_mrf_mix_split(const void* a, const void* b, const void* c, void* y, float slope, int64_t numel, int64_t lo,
                               advh_stream_t stream);
int advh_hifigan_conv_post_split(const void* x, int64_t x_lo, const float* w, float bias, float* wav, int B, int C, int T, int halo,
                                 int k, advh_stream_t stream);

/* ---- LDS line-tile convolution for narrow layers (C_in = C_out = C in {32, 64}) -------------------------------
 * out[m][co] = act(bias[co] + sum_t sum_ci W[t][co][ci] * X[m + toff[t]][ci]) (+ resid[m][co]) over the M rows of a
 * zero-haloed channels-last fp16 map; rows outside the window (h0..h1, w0..w1 of the (Hg, Wg) row grid) are
 * written as zeros, so the output map keeps a zero halo.  X, resid, out_h, out_h2 share one geometry [M][C].
 * Replaces the HiFi-GAN ResBlock1 Conv1d layers of the 64- and 32-channel stages (speechbrain HifiganGenerator via
 * hifigan.py:106-110, 180): toff[t] = (t - (k-1)/2) * dilation.  Weights stay resident in LDS (<= 160 KiB with the
 * double-buffered line buffer: advh_conv_taps_lds_bytes), HBM traffic is input once + output once.               */
typedef struct advh_taps_desc {
    const void* X;        /* fp16 [M][C]                                                          */
    const void* W;        /* fp16 [ntap][C_out][C_in]                                             */
    const float* bias;    /* [C] or NULL                                                          */
    const void* resid;    /* fp16 [M][C] or NULL (added after the activation)                     */
    void* out_h;          /* fp16 [M][C]                                                          */
    void* out_h2;         /* fp16 [M][C] or NULL: LeakyReLU(slope2) of the value stored in out_h   */
    int M, Hg, Wg, h0, h1, w0, w1;
    int ntap;
    int toff[16];
    int act;              /* ADVH_ACT_NONE | ADVH_ACT_LEAKY */
    float slope, slope2;
    int pre_act;          /* 1: LeakyReLU(pre_slope) is applied to X inside the line buffer (X is the raw map) */
    float pre_slope;
} advh_taps_desc;
/* The same layer in the fp32-class mode, C = 64: X, W, resid, out_h, out_h2 are split-format plane pairs (lo plane x_lo / w_lo / r_lo /
 * o_lo elements behind the hi plane; out_h and out_h2 share o_lo), three MFMAs per fragment pair (the arithmetic of the x3 GEMM).  The weights
 * stream tap by tap through a four-slot LDS ring, tap n + 3 requested when tap n starts (two planes of an 11-tap tensor do not fit); there is
 * ONE line buffer, the next tile's lines are requested after the last tap and land under the epilogue.
 * advh_conv_taps_split_tile(C, ntap, span) = positions per tile (256), 0 if the layer does not fit.  pre_act is not supported (ADVH_EUNSUPPORTED).
 * Replaces the x3 implicit GEMM for ResBlock convolutions of HiFi-GAN's 64-channel stage (hifigan.py:106-110, 180): the first of a step from
 * k = 3, the second from k = 7 (gemm.select_conv1d).  */
int advh_conv_taps_split_tile(int C, int ntap, int span);
int advh_conv_taps_split(const advh_taps_desc* d, int C, int64_t x_lo, int64_t w_lo, int64_t r_lo, int64_t o_lo, advh_stream_t stream);
/* 2-D variant: 3x3 stride-1 "same" Conv2d, C_in = C_out = C in {32, 64}, on zero-haloed NHWC fp16 maps of ONE geometry
 * [B][H+2PH][W_+2PW][C] (PH, PW >= 1) -- the second convolution of the U-Net's 32- / 64-channel ConvBlocks
 * (addvisor.py:20-24 with BatchNorm folded).  16 x 16 output tiles with an 18 x 18 line-buffer patch; W [9][C_out][C_in]
 * (tap = kh*3 + kw); only interior positions of out_h are written (its halo must already be zero).                */
typedef struct advh_taps2d_desc {
    const void* X;
    const void* W;
    const float* bias;
    void* out_h;
    int B, H, W_, PH, PW;
    int act;              /* ADVH_ACT_NONE | ADVH_ACT_LEAKY */
    float slope;
} advh_taps2d_desc;
int advh_conv_taps2d_f16(const advh_taps2d_desc* d, int C, advh_stream_t stream);
/* The same layer in the fp32-class mode (csrc/conv_taps2d_x3.hip): X, W, out_h are split-format plane pairs, the lo plane x_lo / w_lo /
 * o_lo elements behind the hi plane (x_lo, o_lo >= one plane of B*(H+2PH)*(W_+2PW)*C elements, w_lo >= 9*C*C, all multiples of 8);
 * W [9][C_out][C_in] per plane (tap = kh*3 + kw); X and out_h distinct.  Three MFMAs per fragment pair in the order and K order of the x3
 * implicit GEMM (gemm.plan_conv2d): the outputs are bit-identical to it.  C = 32: weights resident in LDS; C = 64: streamed tap by tap
 * through an LDS ring.  Only interior positions of out_h are written (both planes' halos must already be zero).  ADVH_EUNSUPPORTED for
 * other C.  advh_conv_taps2d_split_lds_bytes(C) = dynamic LDS per workgroup, -1 for an unsupported C.  */
int advh_conv_taps2d_split_lds_bytes(int C);
int advh_conv_taps2d_split(const advh_taps2d_desc* d, int C, int64_t x_lo, int64_t w_lo, int64_t o_lo, advh_stream_t stream);
/* The 32-channel layer with the U-Net's mask head in its epilogue (d1.block.3 + mask_head, addvisor.py:54-60): instead of storing the
 * 32-channel map the kernel writes logits[b][h][w] = sum_c y[b,h,w,c] * head_w[c] + head_b and mask = sigmoid(logits), fp32 [B][H][W_]
 * (logits may be NULL), where y is the split-format value advh_conv_taps2d_split would have stored (same rounding, same range flag)
 * and the sum runs in advh_unet_head_split's order: the two outputs are bit-identical to that pair of launches.  d->out_h is not
 * used.  ADVH_EUNSUPPORTED for C != 32, ADVH_EINVAL for a NULL head_w / mask and for what advh_conv_taps2d_split rejects.  */
int advh_conv_taps2d_split_head(const advh_taps2d_desc* d, int C, int64_t x_lo, int64_t w_lo, const float* head_w, float head_b,
                                float* mask, float* logits, advh_stream_t stream);
/* Last decoder stage of the U-Net as ONE line-tile launch: up1 = ConvTranspose2d(64,32,(2,1),stride (2,1)) folded into
 * d1.block.0 = Conv2d(33,32,3,padding 1) + BatchNorm + LeakyReLU (addvisor.py:53-54,78-80).
 *   Xc  coarse map  [B][Hc+2PHc][W_+2PWc][64]  fp16, zero halo (PHc, PWc >= 1)              (y2)
 *   Xs  skip map    [B][2Hc+2PHs][W_+2PWs][8]  fp16 = (spectrogram, in-image indicator, 0 x6), zero halo (advh_unet_pack_x)
 *   W   fp16 [2 row parities][15 k-steps][32 rows][32]: per parity the composed weights in the K order
 *       (coarse tap t = 3 ti + tj: 64 channels) x 6, (fine tap kh*3 + kw: 8 channels) x 9, zero-padded 456 -> 480;
 *       row R of a k-step carries output channel 8 ((R>>2)&3) + 4 ((R>>4)&1) + (R&3)
 *   out_h [B][2Hc+2PHo][W_+2PWo][32] fp16, interior written (halo must already be zero); Hc % 8 == 0.            */
typedef struct advh_upconv_desc {
    const void* Xc;
    const void* Xs;
    const void* W;
    const float* bias;    /* [32] or NULL */
    void* out_h;
    int B, Hc, W_, PHc, PWc, PHs, PWs, PHo, PWo;
    int act;              /* ADVH_ACT_NONE | ADVH_ACT_LEAKY */
    float slope;
} advh_upconv_desc;
int advh_upconv21_tile_f16(const advh_upconv_desc* d, advh_stream_t stream);
int advh_upconv21_tile_lds_bytes(void);
/* The same stage in the fp32-class mode (csrc/upconv_tile_x3.hip): Xc, Xs, W, out_h are split-format plane pairs, the lo plane xc_lo /
 * xs_lo / w_lo / o_lo elements behind the hi plane (at least one whole plane, multiples of 8); W per plane as above, [2 row parities][15]
 * [32][32].  Three MFMAs per fragment pair in the order and K order of the x3 implicit GEMM (gemm.plan_upconv2d): the outputs are
 * bit-identical to it.  One row parity per workgroup (its weights resident in LDS), tiles of 32 output rows x 16 columns; any Hc >= 1.
 * Cc = coarse channels, N = output channels: ADVH_EUNSUPPORTED unless (Cc, N) = (64, 32); ADVH_EINVAL for a missing lo plane or a
 * plane distance that is not a multiple of 8.  advh_upconv21_tile_split_lds_bytes() = dynamic LDS per workgroup.  */
int advh_upconv21_tile_split_lds_bytes(void);
int advh_upconv21_tile_split(const advh_upconv_desc* d, int Cc, int N, int64_t xc_lo, int64_t xs_lo, int64_t w_lo, int64_t o_lo,
                             advh_stream_t stream);
/* e2.block.0 of the U-Net as a line-tile launch: Conv2d(32, 64, (5,3), stride (2,1), padding (2,1)) + folded BatchNorm +
 * LeakyReLU (addvisor.py:32).  X [B][2Ho+2PHi][W_+2PWi][32] fp16 zero-haloed (PHi >= 2, PWi >= 1);
 * W fp16 [15 taps = kh*3+kw][64 rows][32 ci], row R of a tap = output channel 32 (R>>5) + 8 ((R>>2)&3) + 4 ((R>>4)&1) + (R&3);
 * out_h [B][Ho+2PHo][W_+2PWo][64], interior written (halo must already be zero).                                      */
typedef struct advh_convs21_desc {
    const void* X;
    const void* W;
    const float* bias;    /* [64] or NULL */
    void* out_h;
    int B, Ho, W_, PHi, PWi, PHo, PWo;
    int act;              /* ADVH_ACT_NONE | ADVH_ACT_LEAKY */
    float slope;
} advh_convs21_desc;
int advh_conv53s21_tile_f16(const advh_convs21_desc* d, advh_stream_t stream);
int advh_conv53s21_tile_lds_bytes(void);
/* The same layer in the fp32-class mode (csrc/conv_s21_tile_x3.hip): X, W, out_h are split-format plane pairs, the lo plane x_lo / w_lo /
 * o_lo elements behind the hi plane (at least one whole plane, multiples of 8).  W per plane [8 k-blocks][64 rows][64]: row R as above,
 * column kk of k-block kb = element 64 kb + kk of the K order (tap kh*3 + kw: 32 channels) x 15, zero-padded 480 -> 512.  Three MFMAs
 * per fragment pair in the order and K order of the x3 implicit GEMM (gemm.plan_conv2d): the outputs are bit-identical to it.  16 x 16
 * output tiles, the weights streamed k-block by k-block through an LDS ring; any Ho >= 1; X and out_h distinct.  Ci = input channels,
 * N = output channels: ADVH_EUNSUPPORTED unless (Ci, N) = (32, 64); ADVH_EINVAL for a missing lo plane or a plane distance that is not
 * a multiple of 8.  advh_conv53s21_tile_split_lds_bytes() = dynamic LDS per workgroup.  */
int advh_conv53s21_tile_split_lds_bytes(void);
int advh_conv53s21_tile_split(const advh_convs21_desc* d, int Ci, int N, int64_t x_lo, int64_t w_lo, int64_t o_lo, advh_stream_t stream);
int advh_conv_taps_tile(int C, int ntap, int span);       /* positions per workgroup tile (128/192/256); 0 = does not fit */
int advh_conv_taps_lds_bytes(int C, int ntap, int span);  /* advh_conv_taps_f16: weights + two line buffers; -1 = does not fit */
int advh_conv_taps_f16(const advh_taps_desc* d, int C, advh_stream_t stream);

/* ---- training step of the U-Net mask decoder (addvisor.py:12-84 under train_addvisor.py:364-378)
 * Maps are zero-haloed channels-last fp16 [B][H+2PH][W+2PW][C]; only interiors are read for statistics / written.
 * BatchNorm2d in training mode (batch statistics over B*H*W, eps 1e-5) around LeakyReLU(slope):
 *   advh_bn_stats     sums[0..C) = sum z, sums[C..2C) = sum (z - mean)^2 >= 0, formed from fp64 sums of z and z^2 (an fp32 sum z^2
 *                     loses mu^2/sigma^2 of its digits to sum z^2 / n - mean^2) and rounded once; deterministic two-stage;
 *                     partial64: advh_bn_partial_count()*2*C DOUBLES -- twice the bytes of every other `partial` here
 *   advh_bn_apply     a = lrelu(coef[c]*z + coef[C+c])                        coef = [scale | shift | mean | invstd], 4*C floats
 *   advh_bn_bwd_sums  with dy^ = g_a * lrelu'(scale*z+shift), z^ = (z-mean)*invstd: sums = [sum dy^ | sum dy^ z^]
 *   advh_bn_bwd_apply dz = coef_b[c]*(dy^ - coef_b[C+c] - z^*coef_b[2C+c]) written at dz + d_c0 + b*d_sB + h*d_sH + w*d_sW
 *                     (interior coordinates; a dense map or the zero-upsampled grid of a strided layer), coef_b = [k1 | m1 | m2].
 *   g_a (same geometry as z) is fp16 or, with g_f32 = 1, fp32: the backward subtracts g_a's per-channel mean, so the
 *   dgrad GEMM that produces it stores its fp32 accumulators (out_f).                                            */
typedef struct advh_map_geom { int B, H, W, C, PH, PW; } advh_map_geom;
int advh_bn_partial_count(void);
/* per-channel coefficients from the reduced sums: forward coef (and the nn.BatchNorm2d train-mode update of the running
 * buffers: momentum, unbiased variance, num_batches_tracked += 1; all three NULL to skip), backward coef_b and the
 * affine gradients dgamma = sum dy^ z^ * inv_scale, dbeta = sum dy^ * inv_scale (n = B*H*W).                       */
int advh_bn_coef(const float* sums, const float* gamma, const float* beta, int C, float n, float eps, float momentum,
                 float* running_mean, float* running_var, int64_t* num_batches_tracked, float* coef, advh_stream_t stream);
int advh_bn_bwd_coef(const float* sums, const float* coef, int C, float n, float inv_scale, float* coef_b, float* dgamma,
                     float* dbeta, advh_stream_t stream);
int advh_bn_stats(const void* z, const advh_map_geom* g, double* partial64, float* sums, advh_stream_t stream);
int advh_bn_apply(const void* z, const advh_map_geom* g, const float* coef, float slope, void* a, advh_stream_t stream);
int advh_bn_bwd_sums(const void* z, const void* g_a, int g_f32, const advh_map_geom* g, const float* coef, float slope,
                     float* partial, float* sums, advh_stream_t stream);
int advh_bn_bwd_apply(const void* z, const void* g_a, int g_f32, const advh_map_geom* g, const float* coef, const float* coef_b, float slope,
                      void* dz, int64_t d_sB, int64_t d_sH, int64_t d_sW, int64_t d_c0, advh_stream_t stream);
/* Operand transpose for the weight-gradient GEMM (reduction over positions needs position-major operands):
 * dst[(t*rpt + r0 + c)*ld + col0 + p] = src[b][PHs + y][PWs + x][c0 + c], p = (b*Hg + hg)*Wg + wg over the layer's common
 * grid, (y, x) = (sy*(hg-GH) + oy[t], sx*(wg-GW) + ox[t]); zero where (y, x) is outside the source interior.  fp16.  */
typedef struct advh_transpose_desc {
    int B, Hg, Wg, GH, GW, H, W;
    int Hs, Ws, PHs, PWs, Cs, c0, nC;
    int sy, sx, ntap, oy[16], ox[16];
    int64_t ld, col0;
    int rpt, r0;          /* dst row of (tap t, channel c) = t*rpt + r0 + c (r0 > 0: second source of a skip concatenation) */
} advh_transpose_desc;
int advh_transpose_gather(const void* src, void* dst, const advh_transpose_desc* d, advh_stream_t stream);
/* mask head backward (addvisor.py:57-60): dlogit = dmask*m*(1-m) (fp32 out), dy1[i][c] = scale*dlogit[i]*w32[c]
 * ([total][32], fp32 if dy_f32 else fp16). */
int advh_unet_head_bwd(const float* dmask, const float* mask, const float* w32, float scale, int64_t total, float* dlogit,
                       void* dy1, int dy_f32, advh_stream_t stream);
/* mask head weight / bias gradient: dw33[c] = sum_i dlogit[i]*y1[i][c] for c < 32, dw33[32] = sum_i dlogit[i]; y1 fp16
 * [total][32]; partial: advh_bn_partial_count()*64 floats; dw33: 64 floats (33 used).                               */
int advh_unet_head_wgrad(const float* dlogit, const void* y1, int64_t total, float* partial, float* dw33, advh_stream_t stream);
/* weight gradient of the 1-channel stem e1.block.0: dw[co][kh*3+kw] = sum dz[b][ho][w][co] * mag[b][2ho+kh-2][w+kw-1];
 * dz = dense fp16 map [B][H/2+2PH][W+2PW][32]; partial: advh_bn_partial_count()*480 floats; dw [32][15] fp32.     */
int advh_unet_stem_wgrad(const void* dz, int Fq, int Tq, int B, int H, int W, const float* mag, int PH, int PW,
                         float* partial, float* dw, advh_stream_t stream);

/* fp32-class training step (train_addvisor.py:363-378 runs the decoder's forward and loss.backward() in fp32): the same
 * kernels on split-format maps [2][B][H+2PH][W+2PW][C] (hi + lo fp16 planes, csrc/device_math.h; `*_lo` = distance in
 * elements between the planes), so LeakyReLU takes the branch the fp32 reference takes and the weight / activation
 * gradients keep ~22 bits.  The convolutions, dgrads and split-K wgrads are advh_gemm_f16 launches with desc.split = 1;
 * advh_transpose_gather is called once per plane.  g_a is a split map here.                                              */
int advh_bn_stats_split(const void* z, int64_t z_lo, const advh_map_geom* g, double* partial64, float* sums, advh_stream_t stream);
int advh_bn_apply_split(const void* z, int64_t z_lo, const advh_map_geom* g, const float* coef, float slope, void* a, int64_t a_lo,
                        advh_stream_t stream);
int advh_bn_bwd_sums_split(const void* z, int64_t z_lo, const void* g_a, int64_t g_lo, const advh_map_geom* g, const float* coef,
                           float slope, float* partial, float* sums, advh_stream_t stream);
int advh_bn_bwd_apply_split(const void* z, int64_t z_lo, const void* g_a, int64_t g_lo, const advh_map_geom* g, const float* coef,
                            const float* coef_b, float slope, void* dz, int64_t dz_lo, int64_t d_sB, int64_t d_sH, int64_t d_sW,
                            int64_t d_c0, advh_stream_t stream);
int advh_unet_head_bwd_split(const float* dmask, const float* mask, const float* w32, float scale, int64_t total, float* dlogit,
                             void* dy1, int64_t dy_lo, advh_stream_t stream);
int advh_unet_head_wgrad_split(const float* dlogit, const void* y1, int64_t y_lo, int64_t total, float* partial, float* dw33,
                               advh_stream_t stream);
int advh_unet_stem_wgrad_split(const void* dz, int64_t dz_lo, int Fq, int Tq, int B, int H, int W, const float* mag, int PH, int PW,
                               float* partial, float* dw, advh_stream_t stream);
/* Weight gradient of the one skip (magnitude) channel of d1.block.0 -- Conv2d(33, 32, 3, padding 1) on torch.cat([up1(y2), x], 1),
 * addvisor.py:57-60, 79: dw[co][kh*3+kw] = sum_p dz[p][co] * mag[b][h+kh-1][w+kw-1] over the H x W crop of mag [B][Fq][Tq]; dz [B][H+2PH][W+2PW][32]
 * (fp16, or a split pair with the lo plane dz_lo elements behind); partial: advh_bn_partial_count() * 288 floats; dw: 288 floats [32][9]. */
int advh_unet_skip_wgrad(const void* dz, int Fq, int Tq, int B, int H, int W, const float* mag, int PH, int PW, float* partial, float* dw,
                         advh_stream_t stream);
int advh_unet_skip_wgrad_split(const void* dz, int64_t dz_lo, int Fq, int Tq, int B, int H, int W, const float* mag, int PH, int PW,
                               float* partial, float* dw, advh_stream_t stream);

/* Weight gradient of a 3x3 stride-1 "same" Conv2d, C_in = C_out = C in {32, 64}, without transposed copies in HBM:
 * dw[kh*3+kw][co][ci] = sum_p dz[p][co] * x[p + (kh-1, kw-1)][ci].  X and DZ are zero-haloed channels-last fp16 maps of
 * the same interior [B][H][W_] with their own halos (>= 1); both MFMA operands are read from LDS tiles with
 * ds_read_b64_tr_b16 (k = position).  partial: advh_conv_wgrad2d_parts(C,B,H,W) * 9*C*C floats of scratch; dw: 9*C*C.  */
typedef struct advh_wgrad2d_desc {
    const void* X;
    const void* DZ;
    float* partial;
    int B, H, W_, PHx, PWx, PHz, PWz;
} advh_wgrad2d_desc;
int advh_conv_wgrad2d_parts(int C, int B, int H, int W);
int advh_conv_wgrad2d_f16(const advh_wgrad2d_desc* d, int C, float* dw, advh_stream_t stream);
/* The same weight gradient in the fp32-class mode, per channel-slice pair: X and DZ are split-format maps (lo plane x_lo / dz_lo elements behind
 * the hi plane) with Cx / Cz channels; the launch computes dw[kh*3+kw][co][ci] for co in [cz0, cz0 + CO), ci in [cx0, cx0 + CI), CI, CO in
 * {32, 64} -- three MFMAs per fragment pair (the arithmetic of the x3 GEMM), fp32 partials (advh_conv_wgrad2d_split_parts(...) * 9*CO*CI floats)
 * and the same fixed-order reduction; dw: 9*CO*CI floats.  A wider layer or one with concatenated sources (addvisor.py:63-75 torch.cat) is covered
 * slice pair by slice pair.  Replaces four operand transposes + a split-K GEMM per layer (train_addvisor.py:376 loss.backward() through
 * addvisor.py:20-24).  */
int advh_conv_wgrad2d_split_parts(int CI, int CO, int B, int H, int W);
int advh_conv_wgrad2d_split(const advh_wgrad2d_desc* d, int CI, int CO, int Cx, int cx0, int Cz, int cz0, int64_t x_lo, int64_t dz_lo,
                            float* dw, advh_stream_t stream);

/* One fused HiFi-GAN ResBlock1 step for the 32- / 64-channel stages (speechbrain HifiganGenerator via hifigan.py:106-110,
 * 180): out = x + conv2(lrelu(conv1(lrelu(x)))) on a zero-haloed channels-last fp16 map [M][C] (rows m with
 * w0 <= m % Wg < w1 are real samples; the others are written as zeros); conv1: k taps, dilation dil, conv2: k taps,
 * dilation 1, both "same"; W1 / W2 [k][C_out][C_in] fp16, b1 / b2 [C] fp32.  The intermediate map stays in LDS.  X and
 * out_h must be different maps.  ADVH_EUNSUPPORTED when both weight tensors + line buffers exceed 160 KiB
 * (advh_resblock_pair_lds_bytes): the caller then launches the two convolutions separately.                         */
typedef struct advh_resblock_desc {
    const void* X;
    const void* W1;
    const float* b1;
    const void* W2;
    const float* b2;
    void* out_h;
    int M, Wg, w0, w1, k, dil;
    float slope;
} advh_resblock_desc;
int advh_resblock_pair_lds_bytes(int C, int k, int dil);
int advh_resblock_pair_f16(const advh_resblock_desc* d, int C, advh_stream_t stream);

/* Concept activation vectors (TCAV, Kim et al. 2018; captum.concept) on flattened activations -- csrc/concept.hip.  All inputs are fp32,
 * row-major with a row stride in floats; every result is bit-identical from run to run (no atomics, one fixed summation order).
 *
 * advh_concept_gram: G[i][j] = sum_f X[i][f] * Y[j][f] for X [M][F] (row stride ldx >= F) and Y [N][F] (ldy >= F); G is double [M][N],
 * contiguous.  F is cut into slabs of S floats, S = max(512, ceil(F / max(1, 1024 / (ceil(M/64) * ceil(N/64)))) rounded up to a multiple
 * of 64): each slab's fp32 partial -- one k-ordered fmaf chain per entry on v_mfma_f32_16x16x4_f32 -- goes to `workspace`
 * (advh_concept_gram_workspace(M, N, F) BYTES, = ceil(F / S) * M * N * 4), and a second launch adds the slabs in ascending order in
 * fp64.  Tails in M, N, F and inside a slab are handled in the kernel.  symmetric = 1 needs Y == X, M == N, ldy == ldx: only the 64 x 64
 * blocks on or above the diagonal are computed and G[i][j], i > j, is G[j][i] bit for bit.  Base pointers and strides that are
 * 16-byte aligned are read with 16-byte loads; anything else (4-byte aligned) with 4-byte loads.
 * ADVH_EINVAL: a null pointer, M, N, F <= 0, M or N > 2^20, F > 2^40, a stride < F, symmetric not in {0, 1} or without Y == X / M == N /
 * ldy == ldx, X / Y / workspace not 4-byte or G not 8-byte aligned.  advh_concept_gram_workspace returns ADVH_EINVAL (negative) for sizes
 * the kernel refuses.
 *
 * advh_concept_combine: W[c][f] = sum_i A[c][i] * X[i][f] for A [C][N] (contiguous) and X [N][F] (stride ldx), W [C][F] (stride ldw):
 * the CAV from the dual coefficients.  One fp32 fmaf chain per output, i ascending from 0.f.  X is read once per group of 8 rows of A.
 * ADVH_EINVAL: a null or misaligned pointer, C, N, F <= 0, a stride < F.
 *
 * advh_concept_time_pool: out[r][h] = sum_t X[r][t][h] for contiguous X [R][T][H], t ascending in fp32 from 0.f; mode 0 = the sum,
 * mode 1 = the sum times float(1 / T).  ADVH_EINVAL: a null pointer, R, T, H <= 0, any other mode.
 * Every argument check precedes the first HIP call.                                                                                  */
int64_t advh_concept_gram_workspace(int M, int N, int64_t F);
int advh_concept_gram(const float* X, int64_t ldx, const float* Y, int64_t ldy, int M, int N, int64_t F, int symmetric, float* workspace,
                      double* G, advh_stream_t stream);
int advh_concept_combine(const float* A, const float* X, int64_t ldx, int C, int N, int64_t F, float* W, int64_t ldw, advh_stream_t stream);
int advh_concept_time_pool(const float* X, int64_t R, int T, int H, int mode, float* out, advh_stream_t stream);

/* Training-data influence (captum.influence: SimilarityInfluence, TracInCPFast; influence functions, Koh & Liang 2017) -- csrc/influence.hip.
 * Rows are fp32, contiguous, with a row stride in floats; every result is bit-identical from run to run (no atomics, one fixed summation
 * order); every argument check precedes the first HIP call.  16-byte loads are issued only where the base pointer and the stride are
 * 16-byte aligned; anything else (4-byte aligned) is read with 4-byte loads.
 *
 * advh_influence_moment: Hm[f][g] = sum_i w[i] * X[i][f] * X[i][g] for X [N][F] (stride ldx >= F); w [N] or NULL (all ones); Hm double
 * [F][F].  The N rows are cut into slabs of S rows, S = max(512, ceil(N / max(1, 1024 / (b (b + 1) / 2))) rounded up to a multiple of 32),
 * b = ceil(F / 64): each slab's fp32 partial -- one i-ordered fmaf chain per entry on v_mfma_f32_16x16x4_f32, the product w[i] * X[i][g]
 * rounded to fp32 first -- goes to `workspace` (advh_influence_moment_workspace(N, F) BYTES, = ceil(N / S) * F * F * 4) and a second
 * launch adds the slabs in ascending order in fp64.  Only the 64 x 64 blocks on or above the diagonal are computed; Hm[f][g], f > g, is
 * Hm[g][f] bit for bit.  ADVH_EINVAL: a null X / workspace / Hm, N outside [1, 2^24], F outside [1, 4096], ldx < F, X / w / workspace not
 * 4-byte or Hm not 8-byte aligned.
 *
 * advh_influence_sqdist: D[i][j] = sum_f (X[i][f] - Y[j][f])^2 for X [M][F], Y [N][F]; D double [M][N].  Direct differences (no
 * a + b - 2 G).  The tiling, the slab length S and the workspace size are advh_concept_gram's (non-symmetric form); within a slab an entry
 * is one fp32 chain acc = fmaf(d, d, acc), d = x - y, f ascending; the slabs are added in ascending order in fp64.  With Y == X (same
 * pointer and stride) the diagonal is exactly 0 and D is bitwise symmetric.  ADVH_EINVAL as advh_concept_gram.
 *
 * advh_influence_sumsq: out[i] = sum_f X[i][f]^2, double [M].  A row is cut into slabs of 16 floats; a slab is one fp32 chain
 * acc = fmaf(x, x, acc), f ascending from 0.f; the slabs are added in ascending order in fp64.  ADVH_EINVAL: a null or misaligned
 * pointer, M outside [1, 2^24], F outside [1, 2^40], ldx < F.
 *
 * advh_influence_residual: out[c][n] = sigma(Z[n][c]) - y[n]; Z double [N][C] (logits: advh_concept_gram of feature rows against
 * checkpoint rows), y float [N] in {0, 1}, out float [C][N].  The sigmoid is fp64 (exp of a non-positive argument only; for y = 1 the
 * difference is formed as -sigma(-z), which does not cancel), rounded once.  ADVH_EINVAL: a null or misaligned pointer, N outside [1, 2^24], C outside [1, 65536].
 *
 * advh_influence_cosine: out[m][n] = G[m][n] / (sqrt(a[m]) * sqrt(b[n])), 0 where a[m] or b[n] is 0 (Captum's cosine_similarity with
 * replace_nan = 0); G double [M][N] contiguous, a double [M], b double [N], out float with row stride ldo >= N; fp64, rounded once.
 * advh_influence_root: out[m][n] = sqrt(D[m][n]) (the euclidean distance from advh_influence_sqdist), fp64, rounded once.
 * advh_influence_scale: out[m][n] = G[m][n] * sum_c (lr[c] * rt[c][m]) * rn[c][n]; c ascending from 0.0 in fp64, every product and sum
 * rounded on its own (no fma), rounded once to fp32.  lr double [C], rt float [C][M], rn float [C][N].  C = 1 with lr = {1} is the
 * influence-function form.  ADVH_EINVAL (all three): a null or misaligned pointer, M outside [1, 2^20], N outside [1, 2^24], ldo < N, C
 * outside [1, 65536].
 * advh_influence_self_scale: out[n] = ss[n] * sum_c (lr[c] * rn[c][n]) * rn[c][n] -- the scale kernel's product on the diagonal (TracIn's
 * self-influence from ss = advh_influence_sumsq), same rounding; ss double [N], out float [N].  ADVH_EINVAL: a null or misaligned pointer,
 * N outside [1, 2^24], C outside [1, 65536].
 *
 * advh_influence_topk: per row m of S float [M][N] (stride lds >= N) the k extreme entries in order -- value descending for largest = 1,
 * ascending for largest = 0, ties to the lower index, -0.0 == +0.0: exactly np.argsort(-+S[m], kind="stable")[:k] on finite input (NaN
 * is not ordered).  idx int32 [M][k], val float [M][k] (the entries of S themselves).  A row is sorted in chunks of 2048 entries that
 * keep k each; the kept entries are sorted again in chunks of 2048 until one chunk is left.  `workspace` holds the kept 8-byte keys of
 * the first two passes: advh_influence_topk_workspace(M, N, k) BYTES = max(16, 8 * M * k * (c1 + c2)), c1 = ceil(N / 2048) counted only
 * if > 1, c2 = ceil(c1 * k / 2048) counted only if c1 > 1 and c2 > 1.  ADVH_EINVAL: a null or misaligned pointer (workspace: 8 bytes),
 * M outside [1, 65535], N outside [1, 2^24], k outside [1, min(N, 256)], lds < N, largest not in {0, 1}.                             */
int64_t advh_influence_moment_workspace(int64_t N, int F);
int advh_influence_moment(const float* X, int64_t ldx, const float* w, int64_t N, int F, float* workspace, double* Hm, advh_stream_t stream);
int64_t advh_influence_sqdist_workspace(int M, int N, int64_t F);
int advh_influence_sqdist(const float* X, int64_t ldx, const float* Y, int64_t ldy, int M, int N, int64_t F, float* workspace, double* D,
                          advh_stream_t stream);
int advh_influence_sumsq(const float* X, int64_t ldx, int M, int64_t F, double* out, advh_stream_t stream);
int advh_influence_residual(const double* Z, const float* y, int64_t N, int C, float* out, advh_stream_t stream);
int advh_influence_cosine(const double* G, const double* a, const double* b, int M, int64_t N, float* out, int64_t ldo, advh_stream_t stream);
int advh_influence_root(const double* D, int M, int64_t N, float* out, int64_t ldo, advh_stream_t stream);
int advh_influence_scale(const double* G, const float* rt, const float* rn, const double* lr, int C, int M, int64_t N, float* out, int64_t ldo,
                         advh_stream_t stream);
int advh_influence_self_scale(const double* ss, const float* rn, const double* lr, int C, int64_t N, float* out, advh_stream_t stream);
int64_t advh_influence_topk_workspace(int M, int64_t N, int k);
int advh_influence_topk(const float* S, int64_t lds, int M, int64_t N, int k, int largest, void* workspace, int* idx, float* val,
                        advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-clip optimised mask explanations (csrc/mask_opt.hip): Fong & Vedaldi's meaningful perturbation (2017) and extremal
 * perturbations (2019) over the STFT mask, restated from the papers (no Captum class exists).  Per clip b the parameters
 * theta[b] [Fc][Tc] live on a coarse grid, K = Fc * Tc; p = 1 / (1 + expf(-theta)); m = U p on [Fm][Tm], U torch's bilinear
 * upsampling (align_corners = False): per axis, fine index d of N reads the coarse points i0, i1 of n with
 *   src = max((d + 0.5) n / N - 0.5, 0), i0 = min(floor(src), n - 1), i1 = min(i0 + 1, n - 1), w1 = src - i0, w0 = 1 - w1
 * (in integers: 2 N src = max((2 d + 1) n - N, 0), i0 its quotient by 2 N and w1 the remainder over 2 N, one correctly rounded
 * fp32 division), and m[f][t] = (p[i0f][i0t] w0t + p[i0f][i1t] w1t) w0f +
 * (p[i1f][i0t] w0t + p[i1f][i1t] w1t) w1f, every product rounded on its own.  All three entry points work on the clips
 * b0 .. b0 + nb - 1 of theta / rank / sign / p / hist (each [B][...]) and on chunk-local rows 2j (mask-in), 2j + 1 (mask-out) of clip
 * b0 + j -- the clip-major layout of advh_istft_masked_rows with S = 2, row0 = 2 b0.  Deterministic: no atomics, a fixed order.
 *
 * advh_mask_opt_rows : rows[2j] = m of clip b0 + j, rows[2j + 1] = 1.f - rows[2j], [2 nb][Fm * Tm].  float4 stores when
 *                      Tm % 4 == 0 and rows is 16-byte aligned, scalar ones otherwise; the same bits either way.
 * advh_mask_opt_terms: one workgroup per clip.  With r_k = 1 when rank[b][k] >= K - K1, else 0 (rank: advh_feature_rank of theta,
 *                      descending = 0),
 *                        A = (1 / K) sum_k (p_k - r_k)^2,  P = (1 / K) sum_k p_k,
 *                        TV = (1 / K) sum_{i, j} (p[i + 1][j] - p[i][j])^2 + (p[i][j + 1] - p[i][j])^2   (pairs inside the grid),
 *                      each sum: thread t adds the cells t, t + 256, ... in that order, then one 256-leaf tree.  From
 *                      z_in = sign[b] logits[2j], z_out = sign[b] logits[2j + 1] and the reward phi (0: z; 1: sigmoid(z);
 *                      2: log sigmoid(z)):
 *                        seeds[2j] = -lam_in sign[b] phi'(z_in),  seeds[2j + 1] = lam_out sign[b] phi'(z_out)
 *                      (dJ / d logit of the two rows: what EmbedderGrad.backward(seed=) takes), p[b][k] = p_k, and
 *                        hist[b][0..5] = (z_in, z_out, A, P, TV, J),
 *                        J = -lam_in phi(z_in) + lam_out phi(z_out) + lam_area A + lam_l1 P + lam_tv TV.
 * advh_mask_opt_step : one wavefront per (clip, cell k).  With G [2 nb][Fm * Tm] the gradient of the rows under those seeds,
 *                        g_k = p_k (1 - p_k) (sum_{(f, t)} U[(f, t), k] (G[2j][f][t] - G[2j + 1][f][t]) + lam_area (2 / K) (p_k - r_k)
 *                              + lam_l1 / K + lam_tv dTV / dp_k),
 *                      the sum over the cell's footprint box row-major, lane l the elements l, l + 64, ..., then a 64-leaf xor
 *                      butterfly; p is read from the terms launch's output (never from a theta another wavefront updates).
 *                      grad_theta[b][k] = g_k when grad_theta != NULL.  optimizer 0 (Adam, torch.optim.Adam's defaults' form):
 *                        m1 = beta1 m1 + (1 - beta1) g, m2 = beta2 m2 + (1 - beta2) g^2,
 *                        theta -= (lr / bias1) m1 / (sqrt(m2) / sqrt(bias2) + eps),  bias_i = 1 - beta_i^step from the host
 *                      (fp32 state and arithmetic; 1 - beta_i, lr / bias1 and sqrt(bias2) are formed in double and rounded once);
 *                      optimizer 1 (SGD): m1 = momentum m1 + g, theta -= lr m1 (m2 unused, may be NULL).  In place.
 * ADVH_EINVAL before any HIP call: a NULL descriptor or pointer (grad_theta and, for SGD, m2 excepted), B, Fm, Tm, Fc, Tc or
 * nb <= 0, B > 65535, Fc > Fm, Tc > Tm, Fm or Tm > 32768, B * K > 2^31 - 1, K1 outside [0, K], a reward outside [0, 2], an optimizer outside
 * [0, 1], a non-finite lr, a clip range outside [0, B), and for Adam a bias correction that is not a positive finite number.   */
typedef struct advh_mask_opt_desc {
    int B;                   /* clips theta, rank, sign, p, the state and a history row hold      */
    int Fm, Tm;              /* the mask                                                          */
    int Fc, Tc;              /* the coarse grid, K = Fc * Tc                                      */
    int K1;                  /* cells the ranked-area template sets to 1                          */
    int reward;              /* 0: logit, 1: prob, 2: log_prob                                    */
    int optimizer;           /* 0: Adam, 1: SGD with momentum                                     */
    float lam_in, lam_out, lam_area, lam_l1, lam_tv;
    double lr, beta1, beta2, eps, momentum; /* double: 1 - beta is formed before the rounding to fp32 */
} advh_mask_opt_desc;
int advh_mask_opt_rows(const advh_mask_opt_desc* d, const float* theta, int b0, int nb, float* rows, advh_stream_t stream);
int advh_mask_opt_terms(const advh_mask_opt_desc* d, const float* theta, const int32_t* rank, const float* sign, const float* logits,
                        int b0, int nb, float* p, float* seeds, float* hist, advh_stream_t stream);
int advh_mask_opt_step(const advh_mask_opt_desc* d, float* theta, const float* p, const int32_t* rank, const float* G, int b0, int nb,
                       double bias1, double bias2, float* m1, float* m2, float* grad_theta, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged batches: per-clip lengths in the embedder forward.  A batch wave [B][L] carries lens[b] valid samples in clip b; the
 * result for clip b is what the model gives for wave[b, :lens[b]] run ALONE, unpadded.  This is the attention_mask semantics
 * of HF Wav2Vec2Model for layer-norm feature encoders (transformers/models/wav2vec2/modeling_wav2vec2.py): the valid frame
 * count per clip is _get_feat_extract_output_lengths / _get_feature_vector_attention_mask; Wav2Vec2Encoder(.StableLayerNorm)
 * .forward sets hidden_states[~expand_attention_mask] = 0 after the projection and adds -inf to the scores of padded keys
 * (the additive attention_mask [B, 1, T, T]).  For group-norm feature encoders HF lets the padding into GroupNorm's
 * statistics; here the statistics run over the clip's own frames in both modes (the per-clip-alone definition).
 *
 * All lengths are int32 [B] DEVICE arrays: `lens` in samples, `frames` in encoder frames (the feature encoder's output-length
 * formula applied to lens[b]).  Every kernel clamps what it reads from them into the batch's own range, so no array content
 * can move an access out of bounds; the host is expected to pass lens[b] in [receptive field, L] and frames[b] in [1, T].
 * The feature-encoder convolutions need no change: they have no padding, so valid frame t of a layer reads valid rows only.
 * Every entry point returns ADVH_EINVAL before any HIP call for a NULL pointer (optional pointers of the sibling excepted),
 * NULL lens / frames, B, T or H <= 0, H % heads != 0 or a bad plane distance, and ADVH_EUNSUPPORTED where its sibling does.
 *
 * advh_w2v2_frontend_ragged / _split_ragged: advh_w2v2_frontend / _split (same arguments, same checks) plus lens.  Per clip the
 *   mean and 1 / (std + 1e-7) run over lens[b] samples (clamped to [10, L]); samples >= lens[b] are never read for their value
 *   (a NaN there does not matter); mode 0: the GroupNorm statistics run over T0_b = (lens[b] - 10) / 5 + 1 frames; rows
 *   t >= T0_b of out are written as zeros, as rows [T0, P0) are in the batch form.  stats_ws / norm_ws / mr_ws hold the
 *   per-clip figures.  lens[b] = L for every b gives the batch form's output bit for bit (n_in >= L).
 * advh_attention_f16_ragged / advh_attention_split_ragged: advh_attention_f16 / _split (same layouts, limits, kernel classes by
 *   the row stride T, error codes) with the keys, queries and tile loops of clip b bounded by Tv = clamp(frames[b], 1, T): rows
 *   t < Tv of ctx are the sibling's result for the clip's first Tv rows alone, rows Tv <= t < T are written as zeros (both
 *   planes); rows >= Tv of qkv are never read for their value.  frames[b] = T gives the sibling's output bit for bit.
 * advh_zero_tail_rows: x [B][T][H] fp32, x[b, frames[b]:, :] = 0 (frames[b] clamped to [0, T]); 16-byte stores where x is
 *   16-byte aligned and H % 4 == 0.  B <= 65535 (ADVH_EUNSUPPORTED above).
 * advh_pool_logreg_ragged: advh_pool_logreg over frames t < frames[b] (clamped to [1, T]), added in the sibling's order and
 *   divided by that count; clips stay T rows apart.                                                                      */
int advh_w2v2_frontend_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                              const float* bias0, const float* gamma, const float* beta, int mode, int normalize, float* stats_ws,
                              float* norm_ws, float* mr_ws, void* out, int T0, int P0, int C0, const int32_t* lens,
                              advh_stream_t stream);
int advh_w2v2_frontend_split_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                    const float* bias0, const float* gamma, const float* beta, int mode, int normalize,
                                    float* stats_ws, float* norm_ws, float* mr_ws, void* out, int64_t out_lo, int T0, int P0, int C0,
                                    const int32_t* lens, advh_stream_t stream);
int advh_attention_f16_ragged(const void* qkv, void* ctx, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);
int advh_attention_split_ragged(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, const int32_t* frames, int B, int T, int H,
                                int heads, advh_stream_t stream);
int advh_zero_tail_rows(float* x, const int32_t* frames, int B, int T, int H, advh_stream_t stream);
int advh_pool_logreg_ragged(const float* h, const float* coef, float intercept, float* logit, float* prob, float* pooled,
                            const int32_t* frames, int B, int T, int H, advh_stream_t stream);

/* ---- ragged batches: the gradient chain (csrc/backward.hip, attention_bwd_x3.hip, attention_bwd_f32.hip, frontend_bwd.hip) -
 * The backward of the ragged forward above, same definition: what the chain returns for clip b is what the batch form returns
 * for wave[b, :lens[b]] run alone.  `lens` / `frames` are the int32 [B] device arrays of the forward, clamped in every kernel.
 * The row-wise launches of the chain (dgrad GEMMs without bias, LayerNorm backward, the feature encoder's dgrad) need no ragged
 * form: a padded row whose incoming gradient is exactly 0, with finite saves, stays exactly 0.  Every entry point returns
 * ADVH_EINVAL before any HIP call for a NULL pointer (optional pointers of the sibling excepted), NULL lens / frames, a
 * non-positive or inconsistent size or a bad plane distance, and ADVH_EUNSUPPORTED where its sibling does.
 *
 * advh_attention_bwd_f16_ragged / advh_attention_bwd_split_ragged: advh_attention_bwd_f16 / _split (same layouts, limits, kernel
 *   instance by the row stride T, refusals, and the split entry honours the attention_bwd_mfma_f32 option) with every bound of
 *   clip b taken from Tv = clamp(frames[b], 1, T): rows t < Tv of dqkv are the sibling's result for the clip's first Tv rows of
 *   qkv / dctx alone, rows Tv <= t < T are written as zeros (every plane), rows >= Tv of qkv / dctx are never read for their
 *   value.  frames[b] = T gives the sibling's output bit for bit.
 * advh_pool_logreg_bwd_ragged / _split_ragged: advh_pool_logreg_bwd / _split with dh[b, t, :] = coef * (dlogit[b] / Tv) for
 *   t < Tv and zeros for Tv <= t < T, in dh and in dh16 (both planes).
 * advh_zero_tail_rows_h: advh_zero_tail_rows for fp16 rows x [B][T][H] (lo = 0) or a plane pair (lo > 0: the lo plane lies lo
 *   elements behind); 16-byte stores where x is 16-byte aligned, H % 8 == 0 and lo % 8 == 0.  B <= 65535.
 * advh_w2v2_frontend_bwd_group_ragged / _split_ragged: advh_w2v2_frontend_bwd_group / _split plus lens: the sums, their divisor
 *   and the bound above which dz0 is written as zero (up to P0) are the clip's own T0_b = (lens[b] - 10) / 5 + 1; samples
 *   >= lens[b] and rows >= T0_b of dy0 are never read for their value.  Same 64-frame tiles and partial order.
 * advh_wave_bwd_ragged: advh_wave_bwd plus lens: the gather, S1 / L_b, (L_b - 1) sigma and T0_b per clip with L_b = lens[b]
 *   (clamped to [10, L]); dx[b, u] = 0 for L_b <= u < n_in.  T0 must be (L - 10) / 5 + 1.  Same 2048-sample tiles.           */
int advh_attention_bwd_f16_ragged(const void* qkv, const void* dctx, void* dqkv, const int32_t* frames, int B, int T, int H, int heads,
                                  advh_stream_t stream);
int advh_attention_bwd_split_ragged(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                    const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);
int advh_pool_logreg_bwd_ragged(const float* coef, const float* dlogit, float* dh, void* dh16, const int32_t* frames, int B, int T,
                                int H, advh_stream_t stream);
int advh_pool_logreg_bwd_split_ragged(const float* coef, const float* dlogit, float* dh, void* dh16, int64_t dh16_lo,
                                      const int32_t* frames, int B, int T, int H, advh_stream_t stream);
int advh_zero_tail_rows_h(void* x, int64_t lo, const int32_t* frames, int B, int T, int H, advh_stream_t stream);
int advh_w2v2_frontend_bwd_group_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                        const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                        const void* dy0, float* part_ws, float* sums_ws, void* dz0, int T0, int P0, int C0,
                                        const int32_t* lens, advh_stream_t stream);
int advh_w2v2_frontend_bwd_group_split_ragged(const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* w0,
                                              const float* gamma, const float* stats_ws, const float* norm_ws, const float* mr_ws,
                                              const void* dy0, int64_t dy_lo, float* part_ws, float* sums_ws, void* dz0, int64_t dz_lo,
                                              int T0, int P0, int C0, const int32_t* lens, advh_stream_t stream);
int advh_wave_bwd_ragged(const float* g, const float* wave, int64_t wave_stride, int n_in, int B, int L, const float* stats_ws,
                         float* dxhat_ws, float* part_ws, int normalize, float out_scale, float* dx, int64_t dx_stride, int T0, int P0,
                         const int32_t* lens, advh_stream_t stream);

/* ---- attention for clips of any length (csrc/attention_long.hip) ----------------------------------------------------------
 * advh_attention_long_f16 / advh_attention_long_split: the layouts of advh_attention_f16 / _split (qkv [B*T][3H], ctx [B*T][H],
 *   fp16 or split plane pairs qkv_lo / ctx_lo elements apart) for ANY T >= 1: the keys stream through LDS in blocks of 256 (112
 *   in the split format at head dims above 64) with an online softmax; grid (heads, B, ceil(T / 128)), one block of 128 queries
 *   per workgroup.  `frames` is an int32 [B] device array or NULL: with it, every bound of clip b is Tv = clamp(frames[b], 1, T)
 *   as in the ragged entry points above (rows t < Tv of ctx: the result for the clip's first Tv rows alone; rows Tv <= t < T:
 *   zeros in every plane; rows >= Tv of qkv are never read for their value); NULL: Tv = T.  ADVH_EINVAL for what the whole-clip
 *   pair reports (frames may be NULL); ADVH_EUNSUPPORTED for dm % 8, dm > 128, B > 65535 or more than 65535 query blocks; both
 *   before any launch.  The whole-clip entry points keep their T <= 256 limit.                                               */
int advh_attention_long_f16(const void* qkv, void* ctx, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);
int advh_attention_long_split(const void* qkv, int64_t qkv_lo, void* ctx, int64_t ctx_lo, const int32_t* frames, int B, int T, int H,
                              int heads, advh_stream_t stream);

/* ---- attention backward for clips of any length (csrc/attention_bwd_long.hip) ---------------------------------------------
 * advh_attention_bwd_long_f16 / advh_attention_bwd_long_split: the layouts of advh_attention_bwd_f16 / _split (qkv and dqkv
 *   [B*T][3H], dctx [B*T][H], fp16 or split plane pairs qkv_lo / dctx_lo / dqkv_lo elements apart) for ANY T >= 1 and head dims
 *   dm = H / heads that are multiples of 8 up to 128, in both formats.  Two kernels on `stream`, no atomics, every product on the
 *   fp32-input matrix instruction: the query kernel (grid (heads, B, ceil(T / 128)); keys streamed in blocks of 128, two sweeps)
 *   writes the softmax statistics (m in the log2 domain, 1 / l, delta) of every query to `stats_ws` and the Q third of dqkv; the
 *   key kernel (grid (heads, B, ceil(T / 128)); queries streamed in blocks of 128 in index order) reads them and writes the K and
 *   V thirds.  stats_ws: fp32 [3][B * heads * T], at least advh_attention_bwd_long_ws_bytes(B, T, heads) bytes, content on entry
 *   irrelevant, 4-byte aligned; it may be shared by consecutive calls on one stream.  Every element of dqkv in rows < T and the
 *   columns of the launch's heads is written.  Split outputs pass the checked conversion (|x| > 65504 saturates and raises the
 *   sticky range flag, advh_split_overflow); fp16 outputs are rounded once.
 *   `frames` is an int32 [B] device array or NULL, with the semantics of advh_attention_long_*: every bound of clip b is
 *   Tv = clamp(frames[b], 1, T) and T stays the row stride; rows t < Tv of dqkv are the result for the clip's first Tv rows alone
 *   (they depend on Tv only, not on T or B), rows Tv <= t < T are zeros in every plane and all three thirds, rows >= Tv of qkv /
 *   dctx / stats_ws are never read.  NULL: Tv = T.
 *   ADVH_EINVAL for a NULL pointer (frames excepted), a non-positive size, H % heads != 0 or, in the split entry, a plane
 *   distance that is not a positive multiple of 8; ADVH_EUNSUPPORTED for dm % 8, dm > 128, B > 65535 or more than 65535 blocks of
 *   128 rows, with dqkv untouched; both before any HIP call.  The whole-clip entry points keep their T <= 256 limit.
 * advh_attention_bwd_long_ws_bytes: 3 * B * heads * T * 4 rounded up to a multiple of 256; 0 for a non-positive argument.  */
size_t advh_attention_bwd_long_ws_bytes(int B, int T, int heads);
int advh_attention_bwd_long_f16(const void* qkv, const void* dctx, void* dqkv, float* stats_ws, const int32_t* frames, int B, int T, int H,
                                int heads, advh_stream_t stream);
int advh_attention_bwd_long_split(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                  float* stats_ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);

/* ---- attention maps, the AH-rule and rollout for clips of any length (csrc/attention_maps_long.hip) ------------------------
 * The streamed forms of advh_attention_maps, advh_attention_bwd_value, advh_rollout_step and advh_rollout_relevance: ANY T >= 1,
 * head dims that are multiples of 8 up to 128, per-clip lengths.  `frames` is an int32 [B] device array or NULL with the semantics
 * of advh_attention_bwd_long_*: every bound of clip b is Tv = clamp(frames[b], 1, T), T stays the stride, what is computed for a
 * clip depends on Tv alone (not on T or B), and rows / columns >= Tv of the inputs are never read.  Every product runs on the
 * fp32-input matrix instruction for both operand formats; no atomics: results are bit-identical from run to run.
 * Both attention entries first launch a statistics kernel (grid (heads, B, ceil(T / 128)); keys streamed in blocks of 128 with an
 * online softmax) that writes (m in the log2 domain, 1 / l) of every query < Tv to planes 0 and 1 of `ws` -- the layout and size
 * of advh_attention_bwd_long_*'s stats_ws (advh_attention_bwd_long_ws_bytes; plane 2 is not touched), content on entry
 * irrelevant, shareable by consecutive calls on one stream -- and then one kernel that recomputes P = exp2(s c2 - m) / l per tile.
 * advh_attention_maps_long: the arguments, semantics and out layout of advh_attention_maps (dctx == NULL: P; otherwise
 *   max(P * (dO V^T * dscale), 0); fuse 0: out [B][heads][T][T], 1 mean / 2 max / 3 min over heads in index order: out [B][T][T]).
 *   A workgroup owns one 128 x 128 tile of one clip's (fuse 0: one head's) map.  Every element of out is written: the clip's map
 *   in the top-left Tv x Tv block, exact zeros elsewhere.  A NaN reaches the elements it enters and wins max and min as it wins
 *   the sum.
 * advh_attention_bwd_value_long: the arguments and contract of advh_attention_bwd_value (dV = P^T dO in the V third through the
 *   checked split conversion; zeros in the Q and K thirds) -- grid (heads, B, ceil(T / 128)), a workgroup owns 128 keys and
 *   streams Q and dO in blocks of 128 rows in index order.  Rows Tv <= t < T of dqkv are zeros in every plane and third.
 * ADVH_EINVAL for what the whole-clip entries report and for a NULL ws (frames may be NULL); ADVH_EUNSUPPORTED for dm % 8,
 *   dm > 128, B > 65535 or more than 65535 blocks of 128 rows, with the output untouched; both before any HIP call, argument errors
 *   first.  The whole-clip entries keep their T <= 256 limit.
 * advh_rollout_step_long: advh_rollout_step's arithmetic with every bound, the contraction included, at Tv; Y is exactly 0
 *   outside its Tv x Tv block.  At frames == NULL and T <= 256 it is bit-equal to advh_rollout_step (same tiles, same k order).
 * advh_rollout_relevance_long: rel[b][j] = (1 / Tv) sum_{i < Tv} X[b][i][j] for j < Tv, rows in order, and 0 for j >= Tv; a grid
 *   over column blocks of 256.  Both: NULL pointers (frames excepted), Y == X, Y == M and B, T <= 0 return ADVH_EINVAL before any
 *   HIP call; B > 65535 or T > 1 048 560 ADVH_EUNSUPPORTED.  */
int advh_attention_maps_long(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, float dscale, int fuse, float* out,
                             float* ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);
int advh_attention_bwd_value_long(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv, int64_t dqkv_lo,
                                  float* ws, const int32_t* frames, int B, int T, int H, int heads, advh_stream_t stream);
int advh_rollout_step_long(const float* M, const float* X, float* Y, float alpha, float beta, float gamma, int normalize,
                           const int32_t* frames, int B, int T, advh_stream_t stream);
int advh_rollout_relevance_long(const float* X, float* rel, const int32_t* frames, int B, int T, advh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged batches in the explanation pipeline (csrc/stft_ragged.hip, csrc/unet_ragged.hip): clip b of a [B][L] buffer gets what
 * it gives when its first lens[b] samples are run alone.  `lens` / `widths` are int32 [B] device arrays; every kernel clamps
 * what it reads from them, so no content moves an access out of the clip's row.  Write L_b = clamp(lens[b], 513, L),
 * T_b = 1 + L_b / hop and W_b = 4 (T_b / 4).
 *
 * advh_stft_forward_ragged: advh_stft_forward's plain forward with `lens` in place of n_in.  wave [B][wave_stride >= L]; the
 *   reflection of clip b happens at L_b; frames t < T_b of X / mag / phase (each may be NULL, not all three) are the sibling's
 *   result for wave[b, :L_b] with L = L_b, bit for bit, frames T_b <= t < T are written as zeros; samples >= L_b are not read.
 *   Optional window, both frames-per-workgroup values, the interior-frame fast path (aligned 8-byte loads) kept.
 * advh_istft_masked_c64_ragged: advh_istft_masked_c64 with per-clip bounds, both branches in one launch (either may be NULL,
 *   not both): frames >= T_b of spec and mask columns >= min(Tm, W_b) count as 0 and are not read; samples [0, L_b) of a
 *   clip's row are the sibling's result on the cropped clip bit for bit, samples [L_b, L) are written as zeros.
 * advh_fmap_clip_tail: x is a zero-haloed NHWC fp16 map [B][H + 2 PH][W + 2 PW][C] (lo = 0) or a split plane pair whose lo
 *   plane lies lo elements behind (lo % 8 == 0, lo >= one plane).  For clip b, every interior row and the interior columns
 *   x >= w_b = clamp(widths[b] >> shift, 0, W): all C channels of every plane are set to 0 with 16-byte stores (C % 8 == 0, x
 *   16-byte aligned); halo rows and columns are not touched, columns < w_b keep their bits.  shift = 0 / 1 / 2 for the full-,
 *   half- and quarter-width maps of the U-Net.  ind_channel >= 0: that channel is also rewritten over the whole interior, 1.0
 *   (hi 1, lo 0) for x < w_b and 0 past it: the in-image indicator of the fused up-convolutions.  < 0: no indicator.
 * advh_zero_tail_cols_f32: x [B][H][W] fp32, t fastest: columns >= clamp(widths[b], 0, W) of every row of clip b are set to 0.
 * Negative codes, all before any HIP call.  ADVH_EINVAL, all four: a NULL or misaligned pointer (optional ones excepted; no
 *   output requested counts as NULL) and bad geometry -- the two STFT entries: what their siblings refuse, wave_stride < L,
 *   T != 1 + L / hop, L <= 512; the map kernel: C % 8, shift outside 0..2, lo % 8 or lo inside the first plane, ind_channel >= C.
 *   ADVH_EUNSUPPORTED: B > 65535 (all four), H > 65535 (advh_fmap_clip_tail), and win spanning more hops than half the frames
 *   per workgroup (advh_istft_masked_c64_ragged only, as its sibling).  The two STFT entries then return ADVH_ENOTINIT without
 *   advh_init.  No scratch, no atomics.                                                                                    */
int advh_stft_forward_ragged(const float* wave, int64_t wave_stride, const int32_t* lens, int B, int L, int hop, int win,
                             const float* window, float* X, float* mag, float* phase, int T, advh_stream_t stream);
int advh_istft_masked_c64_ragged(const float* spec, const float* mask, int Fm, int Tm, int mode, float* wave_in, float* wave_out,
                                 int64_t wave_stride, const int32_t* lens, int B, int T, int L, int hop, int win,
                                 const float* window, advh_stream_t stream);
int advh_fmap_clip_tail(void* x, int64_t lo, const int32_t* widths, int shift, int B, int H, int W, int C, int PH, int PW,
                        int ind_channel, advh_stream_t stream);
int advh_zero_tail_cols_f32(float* x, const int32_t* widths, int B, int H, int W, advh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADDVISOR_HIP_H */
