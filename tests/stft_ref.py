"""fp64 restatement of the framed STFT / ISTFT family of csrc/stft.hip, for the kernel-level tests (tests/test_gpu_stft_kernels.py).

Plain torch, written from the definitions -- index arithmetic, an ``rfft`` / ``irfft`` of each 1024-sample frame and a loop over the
frames for the overlap-add -- not ``torch.stft`` / ``torch.istft`` and not the kernels.  Spectrograms are ``[B, 513, T]`` with
``T = 1 + L // hop`` like the HIP ones.  Every function computes in float64 unless ``dtype`` says otherwise (the GPU tests evaluate
the adjoints once more in float32 as the yardstick of what fp32 arithmetic costs), and everything is differentiable, so autograd
gives the adjoints.  tests/test_stft_ref_cpu.py pins it against ``torch.stft`` / ``torch.istft`` in float64, oracle/signal_ref.py and
the golden vectors.

The second half holds the error measures both test files use; each returns error / bound, so ``<= 1`` passes.
"""
import math

import torch

NFFT = 1024
NBIN = 513
PAD = NFFT // 2

# the project's stated bounds (tests/test_gpu_stft.py, tests/test_gpu_training.py)
TOL_SPEC = 2e-6      # spectra: max |X - X_ref| / max |X_ref|
TOL_WAVE = 5e-6      # waveforms at max |y_ref| ~ 1
TOL_PHASE = 2e-3     # radians, wrap-aware, on bins above 1e-3 of the frame's largest
ADJ_TOL = 1e-4       # adjoints: max |g - g_ref| / max |g_ref|, the hard ceiling


# ---------------------------------------------------------------------------------------------------------------- transforms
def left_of(win):
    """Offset of the ``win``-long window inside the 1024-sample frame (centred, as ``torch.stft`` pads it)."""
    return (NFFT - win) // 2


def window_of(win, window, dtype=torch.float64):
    return torch.ones(win, dtype=dtype) if window is None else window.detach().cpu().to(dtype)


def fit(wave, L, dtype=torch.float64):
    """Zero-pad the tail or crop to ``L`` samples."""
    x = wave.to(dtype)
    n = x.shape[-1]
    return torch.cat([x, x.new_zeros(x.shape[:-1] + (L - n,))], -1) if n < L else x[..., :L]


def reflect_index(L):
    """Source sample of each of the ``L + 1024`` padded samples: reflection about sample 0 and about sample L - 1, the edge
    sample itself not repeated."""
    n = torch.arange(-PAD, L + PAD).abs()
    return torch.where(n >= L, 2 * (L - 1) - n, n)


def frames_rfft(xp, L, hop, win, window=None):
    """``xp [B, L + 1024]`` padded signal -> ``[B, 513, T]``: frame t = padded samples ``[t * hop + left, t * hop + left + win)``
    times the window, placed at ``left`` of a zero 1024-sample frame, rfft."""
    left, T = left_of(win), 1 + L // hop
    w = window_of(win, window, xp.dtype)
    idx = (left + hop * torch.arange(T))[:, None] + torch.arange(win)[None, :]
    buf = xp.new_zeros(xp.shape[:-1] + (T, NFFT))
    buf[..., left:left + win] = xp[..., idx] * w
    return torch.fft.rfft(buf, dim=-1).transpose(-1, -2)


def stft(wave, L, hop, win, window=None, dtype=torch.float64):
    return frames_rfft(fit(wave, L, dtype)[..., reflect_index(L)], L, hop, win, window)


def overlap_add(spec, hop, win, window=None):
    """``spec [B, 513, T]`` complex -> (windowed overlap-added signal ``[B, P]``, envelope ``sum w^2 [P]``) on the padded axis.
    C2R semantics: the imaginary parts of DC and Nyquist are ignored."""
    left, T = left_of(win), spec.shape[-1]
    rdt = spec.real.dtype
    w = window_of(win, window, rdt)
    s = spec.transpose(-1, -2)
    edge = torch.zeros(NBIN, dtype=torch.bool)
    edge[0] = edge[NBIN - 1] = True
    s = torch.where(edge, torch.complex(s.real, torch.zeros_like(s.real)), s)
    fr = torch.fft.irfft(s, n=NFFT, dim=-1)[..., left:left + win] * w
    P = (T - 1) * hop + NFFT
    y = fr.new_zeros(fr.shape[:-2] + (P,))
    env = torch.zeros(P, dtype=rdt)
    for t in range(T):
        a = t * hop + left
        y[..., a:a + win] = y[..., a:a + win] + fr[..., t, :]
        env[a:a + win] += w * w
    return y, env


def normalise(y, env, L):
    """Divide by the envelope where it exceeds 1e-11 (else 0), trim the 512 padding samples, cut to ``L``."""
    ok = env > 1e-11
    out = torch.where(ok, y / torch.where(ok, env, torch.ones_like(env)), torch.zeros_like(y))
    out = out[..., PAD:PAD + L]
    return torch.cat([out, out.new_zeros(out.shape[:-1] + (L - out.shape[-1],))], -1) if out.shape[-1] < L else out


def istft(spec, L, hop, win, window=None):
    y, env = overlap_add(spec, hop, win, window)
    return normalise(y, env, L)


# --------------------------------------------------------------------------------------------------------------------- masks
def embed(mask, T, which=0):
    """The ``(Fm, Tm)`` crop as zeros in ``(513, T)``; ``which = 1`` is ``1 - m`` EVERYWHERE: mask-out passes the bins outside the
    crop unchanged."""
    Fm, Tm = mask.shape[-2:]
    full = mask.new_zeros(mask.shape[:-2] + (NBIN, T))
    full[..., :Fm, :Tm] = mask
    return 1 - full if which else full


def gain(m, M, domain):
    """The factor on X: ``linear`` m; ``log1p`` expm1(m log1p M) / M with the limit m as M -> 0."""
    if domain == "linear":
        return m + 0 * M
    if domain != "log1p":
        raise ValueError(domain)
    pos = M > 0
    Ms = torch.where(pos, M, torch.ones_like(M))
    return torch.where(pos, torch.expm1(m * torch.log1p(Ms)) / Ms, m + 0 * M)


def apply_full(full, X, domain):
    """``X * g(m, |X|) / |X|`` with a full-size mask: exactly 0 where X = 0."""
    return X * gain(full, X.abs(), domain)


def apply_mask(mask, X, domain, which=0):
    """The complex entry: ``mask [.., Fm, Tm]`` on the complex spectrogram ``X [.., 513, T]``."""
    return apply_full(embed(mask.to(X.real.dtype), X.shape[-1], which), X, domain)


def apply_mask_polar(mask, mag, phase, domain, which=0):
    """The polar entry: ``g(m, |X|) e^{i angle X}`` from ``(|X|, angle X)``."""
    full = embed(mask.to(mag.dtype), mag.shape[-1], which)
    a = full * mag if domain == "linear" else torch.expm1(full * torch.log1p(mag))
    return torch.complex(a * torch.cos(phase), a * torch.sin(phase))


def band_swap(spec_a, spec_b, k0, kw, nbands):
    """``[nbands, B, 513, T]``: in band z the bins ``[k0 + z kw, k0 + (z + 1) kw)`` come from ``spec_b``, all others from ``spec_a``."""
    k = torch.arange(NBIN)[:, None]
    return torch.stack([torch.where((k >= k0 + z * kw) & (k < k0 + (z + 1) * kw), spec_b, spec_a) for z in range(nbands)])


def row_clips(rows, B, row0=0, clip_major=0, S=1):
    """The row rule of ``advh_istft_masked_rows``: the clip whose spectrogram launch row r reads, clamped to ``[0, B)``."""
    return [min(max((row0 + r) // S if clip_major else (row0 + r) % B, 0), B - 1) for r in range(rows)]


def masked_istft(mask, X, L, hop, win, window, domain, which=0):
    return istft(apply_mask(mask, X, domain, which), L, hop, win, window)


def masked_istft_polar(mask, mag, phase, L, hop, win, window, domain, which=0):
    return istft(apply_mask_polar(mask, mag, phase, domain, which), L, hop, win, window)


def adjoint(fn, mask, r):
    """``d <fn(m), r> / d m`` by autograd: the vector-Jacobian product of ``m -> fn(m)`` at ``mask``."""
    with torch.enable_grad():
        m = mask.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((fn(m) * r.to(m.dtype)).sum(), m)
    return g.detach()


# ------------------------------------------------------------------------------------------------------------ error measures
def _c(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if torch.is_complex(t) else t.double()


def spec_ratio(got, ref):
    """max |got - ref| over ALL bins / (TOL_SPEC max |ref|)."""
    got, ref = _c(got), _c(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (TOL_SPEC * ref.abs().max())).item()


def wave_ratio(got, ref, scale=1.0):
    """max |got - ref| over ALL samples / (TOL_WAVE scale); ``scale`` = max |y_ref| of the case's unmasked signal, ~ 1."""
    got, ref = _c(got), _c(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (TOL_WAVE * scale)).item()


def adjoint_err(got, ref):
    got, ref = _c(got), _c(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item()


def phase_ratio(phase, X_ref):
    """The project's wrap-aware phase check, per frame: bins above 1e-3 of the FRAME's largest.  Returns (max wrapped
    difference / TOL_PHASE, share of the bins left out among the frames that hold any non-zero sample)."""
    ph, X_ref = _c(phase), _c(X_ref)
    mag = X_ref.abs()
    top = mag.amax(dim=-2, keepdim=True)
    live = (top > 0).expand_as(mag)
    sel = (mag > 1e-3 * top) & live
    if not bool(sel.any()):
        return 0.0, 0.0
    d = torch.remainder((ph - X_ref.angle())[sel] + math.pi, 2 * math.pi) - math.pi
    return (d.abs().max() / TOL_PHASE).item(), 1.0 - sel.sum().item() / live.sum().item()


def hann(win):
    """The periodic Hann window, fp32 as the project builds it."""
    return torch.hann_window(win, periodic=True, dtype=torch.float32)


# (hop, win, windowed): the geometries of the kernel-level tests
GEOMETRIES = {
    "ref": (322, 644, False),
    "oddleft": (321, 642, False),
    "evenhop": (320, 640, False),
    "hann_ref": (322, 644, True),
    "mel": (256, 1024, True),
    "short": (160, 400, True),
    "r4odd": (161, 644, False),
    "r8": (128, 1024, True),
}


def geometry(name):
    hop, win, windowed = GEOMETRIES[name]
    return hop, win, hann(win) if windowed else None


def overlap(hop, win):
    return -(-win // hop)


def grid_boundary_lengths(hop, win, fb):
    """The two lengths that straddle the inverse grid's boundary: the smallest ``L > 512`` with ``(512 + L - left)`` a multiple of
    ``S hop`` (``S = fb - R + 1`` hop segments per workgroup), and ``L + 1``, which needs one more workgroup."""
    left, S = left_of(win), fb - overlap(hop, win) + 1
    assert S >= 1
    L = PAD + 1
    while (PAD + L - left) % (S * hop):
        L += 1
    return L, L + 1
