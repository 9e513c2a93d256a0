"""CPU: pins tests/stft_ref.py, the fp64 restatement the STFT / ISTFT kernel tests compare against.

The transforms against ``torch.stft`` / ``torch.istft`` run in float64 at every geometry of the kernel tests, against
oracle/signal_ref.py and the golden vectors at the reference geometry; the autograd adjoint against the inner-product identity;
the error measures against five structured mistakes a kernel could make, each applied to the fp64 result itself; and the window
check of ``addvisor_hip.ops``."""
import warnings

import numpy as np
import pytest
import torch

import stft_ref as R
from addvisor_hip import ops, synthetic as syn
from oracle import signal_ref

LENGTHS = [513, 16000]
GEOMS = list(R.GEOMETRIES)


def noise(B, n, seed):
    return 0.25 * torch.randn(B, n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def random_spec(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(B, R.NBIN, T, generator=g, dtype=torch.float64),
                         torch.randn(B, R.NBIN, T, generator=g, dtype=torch.float64))


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def torch_window(win, window):
    return torch.ones(win, dtype=torch.float64) if window is None else window.double()


def istft_by_matrix(spec, L, hop, win, window):
    """The inverse from an explicit fp64 frame matrix ``x[n] = (1/N) sum_k c_k Re(X_k e^{2 pi i k n / N})``, c = 1 at DC and
    Nyquist (imaginary parts unused), 2 elsewhere; for the geometries ``torch.istft`` refuses."""
    k = torch.arange(R.NBIN, dtype=torch.float64)[:, None]
    n = torch.arange(R.NFFT, dtype=torch.float64)[None, :]
    ang = 2 * torch.pi * k * n / R.NFFT
    c = torch.full((R.NBIN, 1), 2.0, dtype=torch.float64)
    c[0] = c[-1] = 1.0
    cosm, sinm = c * torch.cos(ang) / R.NFFT, c * torch.sin(ang) / R.NFFT
    sinm[0] = sinm[-1] = 0.0
    fr = spec.real.transpose(-1, -2) @ cosm - spec.imag.transpose(-1, -2) @ sinm          # [B, T, 1024]
    left, T = R.left_of(win), spec.shape[-1]
    w = torch_window(win, window)
    y = torch.zeros(spec.shape[0], (T - 1) * hop + R.NFFT, dtype=torch.float64)
    env = torch.zeros(y.shape[-1], dtype=torch.float64)
    for t in range(T):
        y[:, t * hop + left:t * hop + left + win] += fr[:, t, left:left + win] * w
        env[t * hop + left:t * hop + left + win] += w * w
    out = torch.where(env > 1e-11, y / env.clamp_min(1e-300), torch.zeros_like(y))
    return out[:, R.PAD:R.PAD + L]


# ------------------------------------------------------------------------------------------------------- against torch, fp64
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("geom", GEOMS)
def test_stft_equals_torch_stft_in_float64(geom, L):
    hop, win, window = R.geometry(geom)
    for n_in in (L, L + 777, L - 300):
        w = noise(3, n_in, 1)
        ours = R.stft(w, L, hop, win, window)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = torch.stft(R.fit(w, L), n_fft=R.NFFT, hop_length=hop, win_length=win, window=torch_window(win, window),
                             center=True, pad_mode="reflect", return_complex=True)
        assert ours.shape == ref.shape == (3, R.NBIN, 1 + L // hop)
        assert rel(ours, ref) <= 1e-12, (geom, L, n_in, rel(ours, ref))


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("geom", GEOMS)
def test_istft_equals_torch_istft_in_float64(geom, L):
    """An arbitrary spectrogram (not a signal's transform), DC and Nyquist with imaginary parts."""
    hop, win, window = R.geometry(geom)
    spec = random_spec(3, 1 + L // hop, 2)
    ours = R.istft(spec, L, hop, win, window)
    assert ours.shape == (3, L)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = torch.istft(spec, n_fft=R.NFFT, hop_length=hop, win_length=win, window=torch_window(win, window), center=True,
                              length=L)
        how = "torch.istft"
    except RuntimeError:                                                   # torch's own overlap check refused the geometry
        ref, how = istft_by_matrix(spec, L, hop, win, window), "frame matrix"
    err = rel(ours, ref)
    print(f"istft {geom} L={L} vs {how}: {err:.2e}")
    assert err <= 1e-12, (geom, L, how, err)


def test_istft_equals_the_frame_matrix():
    """The explicit matrix itself, at one geometry torch accepts too, so that the fallback above is pinned either way."""
    hop, win, window = R.geometry("short")
    spec = random_spec(2, 1 + 513 // hop, 3)
    assert rel(R.istft(spec, 513, hop, win, window), istft_by_matrix(spec, 513, hop, win, window)) <= 1e-12


# ------------------------------------------------------------------------------------- against the oracle and the golden vectors
def fp32_close(a, b, what):
    a, b = a.double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= R.TOL_SPEC * scale + 1e-5, (what, err, scale)          # the fp32 oracle's own precision (tests/test_gpu_stft.py)


def test_reference_geometry_equals_the_oracle():
    hop, win, _ = R.geometry("ref")
    L = 16000
    w = syn.make_clips(3, L + 777, seed=7)
    X = R.stft(w, L, hop, win)
    Xo, mago, _ = signal_ref.compute_stft(w, audio_length=1)
    fp32_close(torch.view_as_real(X), torch.view_as_real(Xo), "X")
    fp32_close(X.abs(), mago, "mag")
    assert R.phase_ratio(signal_ref.compute_stft(w, audio_length=1)[2], X)[0] <= 1
    mask = torch.rand(3, 512, 48, generator=torch.Generator().manual_seed(5))
    for domain in ("linear", "log1p"):
        rel_o, irr_o = signal_ref.apply_mask(signal_ref.embed_mask(mask, 513, 50), mago, Xo.angle(), domain)
        for which, spec_o in enumerate((rel_o, irr_o)):
            wo = signal_ref.compute_invert_stft(spec_o, audio_length=1)
            polar = R.masked_istft_polar(mask.double(), mago.double(), Xo.angle().double(), L, hop, win, None, domain, which)
            cplx = R.masked_istft(mask.double(), Xo.to(torch.complex128), L, hop, win, None, domain, which)
            assert (polar - wo).abs().max().item() <= R.TOL_WAVE, (domain, which)
            assert (cplx - wo).abs().max().item() <= R.TOL_WAVE, (domain, which)
    assert torch.equal(R.embed(mask, 50), signal_ref.embed_mask(mask, 513, 50))


def test_reference_geometry_equals_the_golden_vectors(golden):
    hop, win, _ = R.geometry("ref")
    g = golden("stft_1s.npz")
    w = syn.make_clips(1, 16000, seed=21)
    X = R.stft(w, 16000, hop, win)
    fp32_close(X.real, g["X_re"], "X_re")
    fp32_close(X.imag, g["X_im"], "X_im")
    fp32_close(X.abs(), g["mag"], "mag")
    assert R.phase_ratio(torch.from_numpy(g["phase"]), X)[0] <= 1
    assert (R.istft(X, 16000, hop, win) - torch.from_numpy(g["istft"])).abs().max().item() <= R.TOL_WAVE
    for sec in (4, 5):
        g = golden(f"stft_{sec}s.npz")
        L = sec * 16000
        w = syn.make_clips(2, L + 777, seed=22)
        X = R.stft(w, L, hop, win)
        assert tuple(X.shape) == tuple(g["shape"])
        fp32_close(X.real[:, ::19, ::7], g["X_re"], "X_re")
        fp32_close(X.abs()[:, ::19, ::7], g["mag"], "mag")
        assert (R.istft(X, L, hop, win)[:, ::13] - torch.from_numpy(g["istft_roundtrip"])).abs().max().item() <= R.TOL_WAVE
        m = torch.from_numpy(np.random.Generator(np.random.PCG64(23)).uniform(0, 1, size=tuple(X.shape)).astype(np.float32))
        masked = R.masked_istft(m.double(), X, L, hop, win, None, "linear")
        assert (masked[:, ::13] - torch.from_numpy(g["istft_masked"])).abs().max().item() <= R.TOL_WAVE


# ------------------------------------------------------------------------------------------------- masks, bands, rows, adjoint
def test_mask_application_edges():
    X = random_spec(2, 5, 4)
    X[0, :3, :2] = 0
    X[1, 7, 1] = 1e-13
    m = torch.rand(2, 100, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    for domain in ("linear", "log1p"):
        for which in (0, 1):
            Y = R.apply_mask(m, X, domain, which)
            assert bool((Y[0, :3, :2] == 0).all()) and bool(torch.isfinite(torch.view_as_real(Y)).all())
            polar = R.apply_mask_polar(m, X.abs(), X.angle(), domain, which)
            assert rel(polar, Y) <= 1e-12, (domain, which)
        outside = R.apply_mask(m, X, domain, 1)
        assert rel(outside[:, 100:], X[:, 100:]) <= 1e-14 and rel(outside[:, :, 3:], X[:, :, 3:]) <= 1e-14   # mask-out: unchanged
        inside = R.apply_mask(m, X, domain, 0)
        assert bool((inside[:, 100:] == 0).all()) and bool((inside[:, :, 3:] == 0).all())
    assert rel(R.apply_mask(m, X, "log1p")[1, 7, 1], m[1, 7, 1] * X[1, 7, 1]) <= 1e-12                      # the limit m X
    assert rel(R.apply_mask(m, X, "linear", 0) + R.apply_mask(m, X, "linear", 1), X) <= 1e-15


def test_band_swap_and_row_rule():
    a, b = random_spec(2, 3, 7), random_spec(2, 3, 8)
    sw = R.band_swap(a, b, 3, 5, 4)
    assert sw.shape == (4, 2, R.NBIN, 3)
    for z in range(4):
        lo = 3 + 5 * z
        assert torch.equal(sw[z, :, lo:lo + 5], b[:, lo:lo + 5])
        assert torch.equal(sw[z, :, :lo], a[:, :lo]) and torch.equal(sw[z, :, lo + 5:], a[:, lo + 5:])
    assert R.row_clips(5, 2, 3, 0, 1) == [1, 0, 1, 0, 1]                   # the rules of tests/test_gpu_spectral_attr.py
    assert R.row_clips(5, 2, 1, 1, 3) == [0, 0, 1, 1, 1]
    assert R.row_clips(5, 2, 4, 1, 3) == [1, 1, 1, 1, 1]
    assert R.row_clips(3, 3, 1, 1, 1) == [1, 2, 2]


@pytest.mark.parametrize("geom", ["ref", "oddleft", "mel", "short"])
def test_autograd_adjoint_satisfies_the_inner_product_identity(geom):
    """``<istft(m X), r> = <m, adj(r)>``: the masked inverse is linear in m in the ``linear`` domain."""
    hop, win, window = R.geometry(geom)
    L = 1500
    X = random_spec(2, 1 + L // hop, 9)
    gen = torch.Generator().manual_seed(10)
    for Fm, Tm in ((R.NBIN, X.shape[-1]), (512, 4 * (X.shape[-1] // 4))):
        m = torch.rand(2, Fm, Tm, generator=gen, dtype=torch.float64)
        r = torch.randn(2, L, generator=gen, dtype=torch.float64)
        for which in (0, 1):
            fn = lambda mm: R.masked_istft(mm, X, L, hop, win, window, "linear", which)        # noqa: E731
            adj = R.adjoint(fn, m, r)
            lhs = (fn(m) * r).sum() - (fn(torch.zeros_like(m)) * r).sum()                     # which = 1 is affine in m
            rhs = (m * adj).sum()
            assert abs(lhs - rhs).item() <= 1e-12 * max(abs(lhs).item(), (fn(m).abs().max() * r.abs().sum()).item()), (geom, which)


def test_grid_boundary_lengths():
    assert R.grid_boundary_lengths(322, 644, 8) == (1932, 1933)
    assert R.grid_boundary_lengths(322, 644, 16) == (4508, 4509)
    for name, (hop, win, _) in R.GEOMETRIES.items():
        for fb in (8, 16):
            if R.overlap(hop, win) > fb:
                continue
            L, L1 = R.grid_boundary_lengths(hop, win, fb)
            S, left = fb - R.overlap(hop, win) + 1, R.left_of(win)
            n = lambda length: -(-(R.PAD + length - left) // (S * hop))                        # noqa: E731
            assert L > R.PAD and n(L1) == n(L) + 1, (name, fb)


# -------------------------------------------------------------------------------- the error measures reject structured mistakes
def test_error_measures_reject_structured_mistakes():
    """Each mistake is applied to the fp64 result itself, so nothing but the mistake is measured; each must exceed the stated
    bound at least 100-fold (the GPU tests' 8x margin on the adjoints stays two orders below the smallest of them)."""
    L = 16000
    ratios = {}
    for geom in ("ref", "hann_ref", "mel"):
        hop, win, window = R.geometry(geom)
        left, T = R.left_of(win), 1 + L // hop
        w = noise(3, L, 11)
        X = R.stft(w, L, hop, win, window)
        spec = random_spec(3, T, 12)
        y, env = R.overlap_add(spec, hop, win, window)
        spec = spec / R.normalise(y, env, L).abs().max()                  # max |y_ref| = 1
        y, env = R.overlap_add(spec, hop, win, window)
        good = R.normalise(y, env, L)
        assert R.spec_ratio(X, X) == 0 and R.wave_ratio(good, good) == 0

        # 1. a reflection that repeats the edge sample: src = -src - 1 on the left, mirrored on the right
        n = torch.arange(-R.PAD, L + R.PAD)
        n = torch.where(n < 0, -n - 1, n)
        n = torch.where(n >= L, 2 * L - 1 - n, n)
        ratios[geom, "reflection repeats the edge sample"] = R.spec_ratio(R.frames_rfft(R.fit(w, L)[..., n], L, hop, win, window), X)

        # 2. a window shifted by one sample (the rectangular one: placed one sample late in the frame)
        if window is not None:
            shifted = R.stft(w, L, hop, win, torch.roll(window, 1))
            y2, env2 = R.overlap_add(spec, hop, win, torch.roll(window, 1))
            ratios[geom, "window shifted (inverse)"] = R.wave_ratio(R.normalise(y2, env2, L), good)
        else:
            xp = R.fit(w, L)[..., R.reflect_index(L)]
            shifted = R.frames_rfft(torch.roll(xp, -1, -1), L, hop, win)
        ratios[geom, "window shifted (forward)"] = R.spec_ratio(shifted, X)

        # 3. an envelope that omits the last overlapping frame at the clip's end
        ww = R.window_of(win, window) ** 2
        env3 = env.clone()
        a = (T - 1) * hop + left
        env3[a:a + win] -= ww
        ratios[geom, "envelope omits the last frame"] = R.wave_ratio(R.normalise(y, env3, L), good)

        # 4. a waveform whose last hop segment is zero (segments start at thi * hop + left - 512)
        n0 = ((L - 1 + R.PAD - left) // hop) * hop + left - R.PAD
        bad = good.clone()
        bad[:, n0:] = 0
        ratios[geom, "last hop segment zero"] = R.wave_ratio(bad, good)

        # 5. the mask crop embedded one bin too high
        m = torch.rand(3, 512, 4 * (T // 4), generator=torch.Generator().manual_seed(13), dtype=torch.float64)
        full = torch.zeros(3, R.NBIN, T, dtype=torch.float64)
        full[:, 1:513, :m.shape[2]] = m
        for domain in ("linear", "log1p"):
            ok = R.masked_istft(m, spec, L, hop, win, window, domain)
            high = R.istft(R.apply_full(full, spec, domain), L, hop, win, window)
            ratios[geom, f"crop one bin too high ({domain})"] = R.wave_ratio(high, ok)
            adj_ok = R.adjoint(lambda mm: R.masked_istft(mm, spec, L, hop, win, window, domain), m, w)
            adj_high = R.adjoint(lambda mm: R.istft(R.apply_full(torch.nn.functional.pad(mm, (0, T - mm.shape[2], 1, 0)),
                                                                 spec, domain), L, hop, win, window), m, w)
            ratios[geom, f"crop one bin too high (adjoint, {domain}) / ADJ_TOL"] = R.adjoint_err(adj_high, adj_ok) / R.ADJ_TOL
    for (geom, what), ratio in ratios.items():
        print(f"{geom:9s} {what}: {ratio:.3g} x the bound")
    assert all(r >= 100 for r in ratios.values()), {k: v for k, v in ratios.items() if v < 100}


def test_phase_measure():
    X = random_spec(2, 6, 14)
    X[:, :, 5] = 0                                                         # a frame in the zero tail: not counted, not compared
    ph = X.angle()
    assert R.phase_ratio(ph, X) == (0.0, 0.0)
    assert R.phase_ratio(ph + 2 * torch.pi, X)[0] < 1e-9                   # wrap-aware
    off = ph.clone()
    off[1, 200, 2] += 0.01
    assert R.phase_ratio(off, X)[0] > 1
    X[0, :100, 0] *= 1e-6
    ratio, left_out = R.phase_ratio(X.angle(), X)
    assert ratio == 0 and abs(left_out - 100 / (2 * 5 * R.NBIN)) < 1e-12


# --------------------------------------------------------------------------------------------------------- the window check
def test_window_check():
    dev = torch.device("cpu")
    good = torch.hann_window(644, periodic=True)
    assert ops._window(None, 644, dev) is None
    assert ops._window(good, 644, dev) is good
    bad = {
        "float64": good.double(),
        "wrong length": torch.hann_window(642, periodic=True),
        "strided": torch.hann_window(1288, periodic=True)[::2],
        "other device": good,
        "not a tensor": good.tolist(),
    }
    for what, window in bad.items():
        with pytest.raises(ValueError, match="window"):
            ops._window(window, 644, torch.device("cuda:0") if what == "other device" else dev)
    assert ops._window(good.view(1, 644), 644, dev) is not None            # shape is free, the element count is not
