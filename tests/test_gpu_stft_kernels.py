"""GPU: every kernel instance of csrc/stft.hip against the fp64 restatement of tests/stft_ref.py, at the geometries where a framed
transform goes wrong: odd and even window offsets, odd hops, windows with and without a taper, two to eight overlapping frames,
the shortest clip the kernels accept (every frame reflects on both sides), a clip with partial last tiles, and the two lengths
on either side of the inverse grid's boundary.  B = 3 throughout, so the strides of clips b > 0 matter.

Which test reaches which of the 16 instances (FB = ``stft_frames_per_workgroup``, 8 and 16 in every test):

  stft_fwd_kernel<FB, 0>   test_forward, test_forward_unit_impulses                     (ops.stft_forward)
  stft_fwd_kernel<FB, 1>   test_adjoints                                                (ops.istft_masked_bwd, which 0 and 1)
  stft_fwd_kernel<FB, 2>   test_adjoints                                                (ops.istft_masked_rows_bwd)
  istft_kernel<0, FB>      test_masked_inverses                                         (ops.istft_masked: |X|, angle X)
  istft_kernel<1, FB>      test_inverse_of_an_arbitrary_spectrogram                     (ops.istft_complex)
  istft_kernel<2, FB>      test_row_mapped_inverse_and_band_swap                        (ops.istft_bandswap)
  istft_kernel<3, FB>      test_masked_inverses, test_adjoints (inner product)          (ops.istft_masked_c64)
  istft_kernel<4, FB>      test_row_mapped_inverse_and_band_swap, test_adjoints (inner product)   (ops.istft_masked_rows)
  the R > FB / 2 refusal   test_eight_overlapping_frames_are_refused_at_fb_8

Bounds: the project's stated ones (stft_ref.TOL_SPEC, TOL_WAVE, TOL_PHASE, ADJ_TOL), spectra WITHOUT the absolute 1e-5 term the
fp32 oracle needed.  The adjoints are also held to 8x the error of the same operation evaluated by torch in fp32 on the CPU
(or 1e-6 of max |ref| where that is larger): the margin for another summation order, the table twiddles and the hardware
log / exp of the mask factor; tests/test_stft_ref_cpu.py shows the structured mistakes two orders above it.  Every test prints
its worst error / bound."""
import pytest
import torch

import stft_ref as R
from addvisor_hip import _lib, ops

pytestmark = pytest.mark.gpu

B = 3
FBS = [8, 16]
DOMAINS = ["linear", "log1p"]
CASES = [(g, fb) for g in R.GEOMETRIES for fb in FBS]
INVERSE_CASES = [(g, fb) for g, fb in CASES if R.overlap(*R.GEOMETRIES[g][:2]) <= fb // 2]      # launch_istft: R <= FB / 2
ROW_CASES = [(g, fb) for g in ("oddleft", "mel") for fb in FBS]
ids = lambda cases: [f"{g}-fb{fb}" for g, fb in cases]                                           # noqa: E731

_REF = {}


def ref_of(key, fn):
    """An fp64 reference, computed once and shared by the two FB values."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.fixture
def frames_per_workgroup():
    def set_fb(fb):
        assert _lib.lib().advh_set_option(b"stft_frames_per_workgroup", fb) == 0
    yield set_fb
    set_fb(8)


def seed_of(*parts):
    """A seed from small integers."""
    s = 17
    for p in parts:
        s = (s * 1000003 + int(p)) % (2 ** 31 - 1)
    return s


def lengths(geom, fb):
    hop, win, _ = R.GEOMETRIES[geom]
    return [513, 16000, *R.grid_boundary_lengths(hop, win, fb)]


def on(dev, t):
    return None if t is None else t.to(dev)


def random_spec(T, seed, rows=B):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(rows, R.NBIN, T, generator=g, dtype=torch.float64),
                         torch.randn(rows, R.NBIN, T, generator=g, dtype=torch.float64))


def crops_of(T, which=((513, None), (512, -4), (100, 7), (1, 1))):
    """The four mask crops, clipped to T; ``(512, 4 (T // 4))`` drops out where T < 4."""
    out = []
    for Fm, Tm in which:
        Tm = T if Tm is None else 4 * (T // 4) if Tm == -4 else min(Tm, T)
        if Tm >= 1 and (Fm, Tm) not in out:
            out.append((Fm, Tm))
    return out


def random_mask(rows, Fm, Tm, seed):
    """Uniform in [0, 1] with a block of exact zeros (row 0) and a block of exact ones (row 1)."""
    m = torch.rand(rows, Fm, Tm, generator=torch.Generator().manual_seed(seed))
    m[0, :max(1, Fm // 3), :max(1, Tm // 2)] = 0.0
    m[1, Fm // 2:, :] = 1.0
    return m


# -------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("geom,fb", CASES, ids=ids(CASES))
def test_forward(gpu_device, frames_per_workgroup, geom, fb):
    """X, |X| and |X| e^{i phase} over ALL bins; crop, odd and even row stride, a zero tail the right-hand reflection reads back, an
    almost empty clip; the calls for fewer outputs bit for bit."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd = on(gpu_device, window)
    worst = {"X": 0.0, "mag": 0.0, "polar": 0.0, "phase": 0.0, "left out": 0.0}
    for L in lengths(geom, fb):
        for n_in in (L, L + 777, L - 300, L - 301, 5):
            w = 0.25 * torch.randn(B, n_in, generator=torch.Generator().manual_seed(seed_of(L, n_in)))
            Xr = ref_of(("fwd", geom, L, n_in), lambda: R.stft(w, L, hop, win, window))
            X, mag, ph = ops.stft_forward(w.to(gpu_device), L, hop, win, window=wd)
            assert X.shape == Xr.shape and mag.shape == Xr.shape and ph.shape == Xr.shape
            polar = torch.polar(mag.double(), ph.double())
            pr, left_out = R.phase_ratio(ph, Xr)
            for name, ratio in (("X", R.spec_ratio(X, Xr)), ("mag", R.spec_ratio(mag, Xr.abs())), ("polar", R.spec_ratio(polar, Xr)),
                                ("phase", pr), ("left out", left_out / 0.01)):
                worst[name] = max(worst[name], ratio)
                assert ratio <= 1, (geom, fb, L, n_in, name, ratio)
            dead = (Xr.abs().amax(dim=1) == 0).to(gpu_device)             # [B, T]: frames entirely in the zero tail
            assert not (n_in == 5 and L == 16000) or bool(dead.any())
            for name, t in (("X", X.abs()), ("mag", mag), ("phase", ph)):
                assert bool((t.transpose(1, 2)[dead] == 0).all()), (geom, fb, L, n_in, name, "zero-tail frame not exactly 0")
            assert bool((X[:, 0].imag == 0).all()) and bool((X[:, 512].imag == 0).all())
            if n_in in (L, L - 301):
                only_x = ops.stft_forward(w.to(gpu_device), L, hop, win, window=wd, want_mag=False, want_phase=False)
                only_mag = ops.stft_forward(w.to(gpu_device), L, hop, win, window=wd, want_complex=False, want_phase=False)
                assert only_x[1] is None and only_x[2] is None and only_mag[0] is None and only_mag[2] is None
                assert torch.equal(torch.view_as_real(only_x[0]), torch.view_as_real(X)) and torch.equal(only_mag[1], mag)
    print(f"forward {geom} FB={fb}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("geom,fb", CASES, ids=ids(CASES))
def test_forward_unit_impulses(gpu_device, frames_per_workgroup, geom, fb):
    """One unit impulse per clip, at samples 0, 1, L - 1 and mid-clip: every bin of a frame has the modulus of the window sample
    the impulse falls on, so the reflection and the frame placement are judged bin by bin with nothing hidden under a neighbour."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd, left = on(gpu_device, window), R.left_of(win)
    wv = R.window_of(win, window)
    worst = 0.0
    for L in lengths(geom, fb):
        mid = L // 2 + 3
        pos = [0, 1, L - 1, mid]
        w = torch.zeros(len(pos), L)
        for i, p in enumerate(pos):
            w[i, p] = 1.0
        Xr = ref_of(("impulse", geom, L), lambda: R.stft(w, L, hop, win, window))
        X, mag, _ = ops.stft_forward(w.to(gpu_device), L, hop, win, window=wd)
        for ratio in (R.spec_ratio(X, Xr), R.spec_ratio(mag, Xr.abs())):
            worst = max(worst, ratio)
            assert ratio <= 1, (geom, fb, L, ratio)
        if mid >= R.PAD and mid + R.PAD < L:                               # seen once by every frame: no reflected copy
            j = mid + R.PAD - left - hop * torch.arange(1 + L // hop)
            want = torch.where((j >= 0) & (j < win), wv[j.clamp(0, win - 1)], torch.zeros((), dtype=torch.float64))
            err = (mag[3].double().cpu() - want[None, :]).abs().max().item()
            worst = max(worst, err / (R.TOL_SPEC * want.max().item()))
            assert err <= R.TOL_SPEC * want.max().item(), (geom, fb, L, err)
    print(f"impulses {geom} FB={fb}: worst error / bound {worst:.3f}")


# -------------------------------------------------------------------------------------------------------------------- inverse
@pytest.mark.parametrize("geom,fb", INVERSE_CASES, ids=ids(INVERSE_CASES))
def test_inverse_of_an_arbitrary_spectrogram(gpu_device, frames_per_workgroup, geom, fb):
    """A random complex spectrogram -- not the transform of any signal, DC and Nyquist with imaginary parts -- scaled to
    max |y_ref| = 1, compared over all samples, the first and last hop included."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd = on(gpu_device, window)
    worst = 0.0
    for L in lengths(geom, fb):
        def make():
            s = random_spec(1 + L // hop, seed_of(L, 1))
            s = (s / R.istft(s, L, hop, win, window).abs().max()).to(torch.complex64)
            return s, R.istft(s.to(torch.complex128), L, hop, win, window)
        spec, yr = ref_of(("c64", geom, L), make)
        assert bool((spec[:, 0].imag != 0).all()) and bool((spec[:, 512].imag != 0).all())
        y = ops.istft_complex(spec.to(gpu_device), L, hop, win, window=wd)
        ratio = R.wave_ratio(y, yr, yr.abs().max().item())
        worst = max(worst, ratio)
        assert y.shape == (B, L) and ratio <= 1, (geom, fb, L, ratio)
    print(f"istft_complex {geom} FB={fb}: worst error / bound {worst:.3f}")


def special_spec(T, seed):
    """Unit-variance complex noise with exact zeros and bins of modulus 1e-13, 1e-9 and 1e3 (frames 0 and 1: every T has them)."""
    s = random_spec(T, seed)
    unit = s / s.abs()
    s[0, 5:9, 0] = 0
    s[1, 200:203, :] = 0
    s[2, 0, 1] = 0
    for b in range(B):
        s[b, 20 + b, 0] = 1e-13 * unit[b, 20 + b, 0]
        s[b, 0, 0] = 1e-13
        s[b, 30 + b, 1] = 1e-9 * unit[b, 30 + b, 1]
        s[b, 40 + b, 1] = 1e3 * unit[b, 40 + b, 1]
    s[0, 0, 0] = 1e3
    return s.to(torch.complex64)


@pytest.mark.parametrize("geom,fb", INVERSE_CASES, ids=ids(INVERSE_CASES))
def test_masked_inverses(gpu_device, frames_per_workgroup, geom, fb):
    """Both entry points, both domains, four crops, both outputs against fp64; one-output calls bit for bit; linear in + out =
    the unmasked inverse; the polar and the complex entry within the waveform bound of each other."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd, d = on(gpu_device, window), gpu_device
    worst = 0.0
    for L in lengths(geom, fb):
        T = 1 + L // hop
        X = special_spec(T, seed_of(L, 2))
        mag, ph = X.abs(), X.angle()
        X64, mag64, ph64 = X.to(torch.complex128), mag.double(), ph.double()
        plain = ref_of(("plain", geom, L), lambda: R.istft(X64, L, hop, win, window))
        scale = plain.abs().max().item()                                   # max |y_ref| of the unmasked signal
        Xd, magd, phd = X.to(d), mag.to(d), ph.to(d)
        for domain in DOMAINS:
            for Fm, Tm in crops_of(T):
                m = random_mask(B, Fm, Tm, seed_of(L, Fm, Tm))
                md, m64 = m.to(d), m.double()
                refs = ref_of(("masked", geom, L, domain, Fm, Tm), lambda: (
                    [R.masked_istft_polar(m64, mag64, ph64, L, hop, win, window, domain, z) for z in (0, 1)],
                    [R.masked_istft(m64, X64, L, hop, win, window, domain, z) for z in (0, 1)]))
                p_io = ops.istft_masked(magd, phd, md, L, domain=domain, hop=hop, win=win, window=wd)
                c_io = ops.istft_masked_c64(Xd, md, L, domain=domain, hop=hop, win=win, window=wd)
                case = (geom, fb, L, domain, (Fm, Tm))
                for z in (0, 1):
                    for got, ref in ((p_io[z], refs[0][z]), (c_io[z], refs[1][z]), (c_io[z], p_io[z])):
                        ratio = R.wave_ratio(got, ref, scale)
                        worst = max(worst, ratio)
                        assert got.shape == (B, L) and ratio <= 1, (case, z, ratio)
                kw = dict(domain=domain, hop=hop, win=win, window=wd)
                assert torch.equal(ops.istft_masked(magd, phd, md, L, want_out=False, **kw)[0], p_io[0]), case
                assert torch.equal(ops.istft_masked(magd, phd, md, L, want_in=False, **kw)[1], p_io[1]), case
                assert torch.equal(ops.istft_masked_c64(Xd, md, L, want_out=False, **kw)[0], c_io[0]), case
                assert torch.equal(ops.istft_masked_c64(Xd, md, L, want_in=False, **kw)[1], c_io[1]), case
                if domain == "linear":                                     # two results, each within the bound
                    for io in (p_io, c_io):
                        ratio = R.wave_ratio(io[0] + io[1], plain, 2 * scale)
                        worst = max(worst, ratio)
                        assert ratio <= 1, (case, "in + out", ratio)
    print(f"masked inverses {geom} FB={fb}: worst error / bound {worst:.3f}")


ROW_RULE = dict(row0=1, clip_major=1, S=1)                                 # rows -> clips 1, 2, 3 clamped to 2


@pytest.mark.parametrize("geom,fb", ROW_CASES, ids=ids(ROW_CASES))
def test_row_mapped_inverse_and_band_swap(gpu_device, frames_per_workgroup, geom, fb):
    """SRC 4 (three rows, the last one clamped) and SRC 2 (k0 = 3, kw = 5, four bands) at an odd window offset and at four
    overlapping frames; the reference geometry has them in tests/test_gpu_spectral_attr.py and tests/test_gpu_bandswap.py."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd, d = on(gpu_device, window), gpu_device
    clips = R.row_clips(3, B, **ROW_RULE)
    assert clips == [1, 2, 2]
    worst = 0.0
    for L in lengths(geom, fb):
        T = 1 + L // hop

        def make():
            a, b = random_spec(T, seed_of(L, 3)), random_spec(T, seed_of(L, 4))
            s = R.istft(a, L, hop, win, window).abs().max()
            return (a / s).to(torch.complex64), (b / s).to(torch.complex64)
        a, b = ref_of(("ab", geom, L), make)
        a64, b64 = a.to(torch.complex128), b.to(torch.complex128)
        Fm, Tm = crops_of(T)[1] if T >= 4 else crops_of(T)[0]
        m = random_mask(3, Fm, Tm, seed_of(L, 5))
        for domain in DOMAINS:
            ref = ref_of(("rows", geom, L, domain), lambda: R.masked_istft(m.double(), a64[clips], L, hop, win, window, domain))
            got = ops.istft_masked_rows(a.to(d), m.to(d), L, domain, hop=hop, win=win, window=wd, **ROW_RULE)
            ratio = R.wave_ratio(got, ref)
            worst = max(worst, ratio)
            assert got.shape == (3, L) and ratio <= 1, (geom, fb, L, domain, ratio)
        ref = ref_of(("bands", geom, L), lambda: R.istft(R.band_swap(a64, b64, 3, 5, 4), L, hop, win, window))
        got = ops.istft_bandswap(a.to(d), b.to(d), L, k0=3, kw=5, nbands=4, hop=hop, win=win, window=wd)
        ratio = R.wave_ratio(got, ref)
        worst = max(worst, ratio)
        assert got.shape == (4, B, L) and ratio <= 1, (geom, fb, L, "band swap", ratio)
    print(f"rows and band swap {geom} FB={fb}: worst error / bound {worst:.3f}")


def test_eight_overlapping_frames_are_refused_at_fb_8(gpu_device, frames_per_workgroup):
    """R = 8 > FB / 2 at FB = 8: every inverse entry point reports "unsupported" before any launch (test_forward has the forward
    of this geometry at both FB values, the other tests its inverses at FB = 16)."""
    frames_per_workgroup(8)
    hop, win, window = R.geometry("r8")
    assert R.overlap(hop, win) == 8
    L, d = 16000, gpu_device
    T = 1 + L // hop
    X = random_spec(T, 6).to(torch.complex64).to(d)
    m = torch.rand(B, 512, 4 * (T // 4), generator=torch.Generator().manual_seed(7)).to(d)
    kw = dict(hop=hop, win=win, window=window.to(d))
    calls = [
        lambda: ops.istft_complex(X, L, **kw),
        lambda: ops.istft_masked(X.abs(), X.angle(), m, L, domain="linear", **kw),
        lambda: ops.istft_masked(X.abs(), X.angle(), None, L, domain="none", want_out=False, **kw),
        lambda: ops.istft_masked_c64(X, m, L, domain="log1p", **kw),
        lambda: ops.istft_masked_rows(X, m, L, "linear", **kw),
        lambda: ops.istft_bandswap(X, X, L, k0=3, kw=5, nbands=4, hop=hop, win=win, window=kw["window"]),
    ]
    for call in calls:
        with pytest.raises(_lib.AdvhError, match="UNSUPPORTED"):
            call()


# ------------------------------------------------------------------------------------------------------------------- adjoints
def adjoint_bound(ref32, ref64):
    """8x what torch's own fp32 evaluation of the operation loses against fp64, or 1e-6 of max |ref| where that is larger."""
    return max(8 * R.adjoint_err(ref32, ref64), 1e-6)


@pytest.mark.parametrize("geom,fb", INVERSE_CASES, ids=ids(INVERSE_CASES))
def test_adjoints(gpu_device, frames_per_workgroup, geom, fb):
    """``ops.istft_masked_bwd`` (both branches) and ``ops.istft_masked_rows_bwd`` against fp64 autograd of the restatement, held to
    ADJ_TOL and to the fp32 yardstick; in the linear domain also ``<istft(m), r> = <m, adj(r)>`` against the HIP forward, summed
    in fp64 on the host (the mask-out branch is affine in m: its value at m = 0 is subtracted)."""
    frames_per_workgroup(fb)
    hop, win, window = R.geometry(geom)
    wd, d = on(gpu_device, window), gpu_device
    clips = R.row_clips(3, B, **ROW_RULE)
    worst = {"vs fp64 / ADJ_TOL": 0.0, "vs fp64 / fp32 yardstick": 0.0, "inner product / ADJ_TOL": 0.0}
    yardstick = [1.0, 0.0]                                                 # smallest and largest fp32-torch error met

    def judge(got, refs, case):
        ref64, ref32 = refs
        err = R.adjoint_err(got, ref64)
        bound = adjoint_bound(ref32, ref64)
        e32 = R.adjoint_err(ref32, ref64)
        yardstick[:] = [min(yardstick[0], e32), max(yardstick[1], e32)]
        worst["vs fp64 / ADJ_TOL"] = max(worst["vs fp64 / ADJ_TOL"], err / R.ADJ_TOL)
        worst["vs fp64 / fp32 yardstick"] = max(worst["vs fp64 / fp32 yardstick"], err / bound)
        assert got.shape == ref64.shape and err <= R.ADJ_TOL and err <= bound, (case, err, bound)

    def inner(lhs_wave, r, m, adj, case):
        lhs = (lhs_wave.double().cpu() * r.double()).sum(1)
        rhs = (m.double() * adj.double().cpu()).flatten(1).sum(1)
        err = ((lhs - rhs).abs().max() / lhs.abs().max()).item()
        worst["inner product / ADJ_TOL"] = max(worst["inner product / ADJ_TOL"], err / R.ADJ_TOL)
        assert err <= R.ADJ_TOL, (case, lhs.tolist(), rhs.tolist(), err)

    for L in (513, 16000):
        T = 1 + L // hop
        g = torch.Generator().manual_seed(seed_of(L, 8))
        X = random_spec(T, seed_of(L, 9)).to(torch.complex64)
        mag, ph = X.abs(), X.angle()
        r = torch.randn(B, L, generator=g)
        Xd, magd, phd, rd = X.to(d), mag.to(d), ph.to(d), r.to(d)
        for Fm, Tm in crops_of(T, ((513, None), (512, -4))):
            m = torch.rand(B, Fm, Tm, generator=g)
            md = m.to(d)
            for domain in DOMAINS:
                kw = dict(domain=domain, hop=hop, win=win, window=wd)

                def both(fn64, fn32):
                    return R.adjoint(fn64, m.double(), r.double()), R.adjoint(fn32, m, r)
                for which in (0, 1):
                    case = (geom, fb, L, (Fm, Tm), domain, which)
                    refs = ref_of(("adj1", geom, L, Fm, Tm, domain, which), lambda: both(
                        lambda mm: R.masked_istft_polar(mm, mag.double(), ph.double(), L, hop, win, window, domain, which),
                        lambda mm: R.masked_istft_polar(mm, mag, ph, L, hop, win, window, domain, which)))
                    got = ops.istft_masked_bwd(rd, magd, phd, md, which, **kw)
                    judge(got, refs, case)
                    if domain == "linear":
                        io = ops.istft_masked(magd, phd, md, L, **kw)
                        lhs = io[which] - ops.istft_masked(magd, phd, torch.zeros_like(md), L, **kw)[which] if which else io[0]
                        inner(lhs, r, m, got, case)
                case = (geom, fb, L, (Fm, Tm), domain, "rows")
                refs = ref_of(("adj2", geom, L, Fm, Tm, domain), lambda: both(
                    lambda mm: R.masked_istft(mm, X.to(torch.complex128)[clips], L, hop, win, window, domain),
                    lambda mm: R.masked_istft(mm, X[clips], L, hop, win, window, domain)))
                got = ops.istft_masked_rows_bwd(rd, Xd, md, domain, hop=hop, win=win, window=wd, **ROW_RULE)
                judge(got, refs, case)
                if domain == "linear":
                    rows = ops.istft_masked_rows(Xd, md, L, domain, hop=hop, win=win, window=wd, **ROW_RULE)
                    inner(rows, r, m, got, case)
                    c64 = ops.istft_masked_c64(Xd[clips].contiguous(), md, L, want_out=False, **kw)[0]
                    assert torch.equal(rows, c64), case
    print(f"adjoints {geom} FB={fb}: worst " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items())
          + f"; torch fp32 on the CPU {yardstick[0]:.2e} ... {yardstick[1]:.2e}")
