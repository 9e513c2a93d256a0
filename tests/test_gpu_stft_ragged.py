"""GPU: advh_stft_forward_ragged and advh_istft_masked_c64_ragged (csrc/stft_ragged.hip) on the shared length table of
tests/ragged_explain_ref.py, nine clips in one launch with NaN-prefilled outputs, at both frames-per-workgroup values, the reference
geometry (hop 322, win 644, rectangular) and a windowed one (hop 256, win 1024, Hann).

Per clip: against the fp64 restatement of tests/stft_ref.py (forward) / ``torch.istft(length=n_b)`` of the fp64 masked spectrum
(inverse) at the bars of the existing STFT tests (stft_ref.TOL_SPEC, TOL_WAVE); bit for bit against the batch entry point on the
cropped clip; exact zeros past the clip; NaN / 1e30 past the clip's extent change no bit."""
import pytest
import torch

import ragged_explain_ref as E
import stft_ref as R
from addvisor_hip import _lib, ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GEOMS = {"ref": (322, 644, False), "mel": (256, 1024, True)}
CASES = [(g, fb) for g in GEOMS for fb in (8, 16)]
L, LENS, B = E.L, list(E.LENGTHS), len(E.LENGTHS)


@pytest.fixture
def frames_per_workgroup():
    def set_fb(fb):
        assert _lib.lib().advh_set_option(b"stft_frames_per_workgroup", fb) == 0
    yield set_fb
    set_fb(8)


def geometry(name, dev):
    hop, win, windowed = GEOMS[name]
    window = R.hann(win) if windowed else None
    return hop, win, window, None if window is None else window.to(dev)


def counts(hop):
    return [E.frame_counts(n, hop) for n in LENS]


def forward_raw(w, lens_d, hop, win, wd, T):
    """The entry point itself, on NaN-prefilled outputs."""
    X, mag, ph = (torch.full(s, float("nan"), device=w.device) for s in ((B, 513, T, 2), (B, 513, T), (B, 513, T)))
    rc = _lib.lib().advh_stft_forward_ragged(w.data_ptr(), w.stride(0), lens_d.data_ptr(), B, L, hop, win, None if wd is None else wd.data_ptr(),
                                             X.data_ptr(), mag.data_ptr(), ph.data_ptr(), T, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "advh_stft_forward_ragged")
    return X, mag, ph


@pytest.mark.parametrize("geom,fb", CASES, ids=[f"{g}-fb{fb}" for g, fb in CASES])
def test_forward(gpu_device, frames_per_workgroup, geom, fb):
    _lib.init()
    frames_per_workgroup(fb)
    hop, win, window, wd = geometry(geom, gpu_device)
    T = 1 + L // hop
    w = E.clips().to(gpu_device)
    lens_d = torch.tensor(LENS, dtype=torch.int32, device=gpu_device)
    X, mag, ph = forward_raw(w, lens_d, hop, win, wd, T)
    assert not torch.isnan(X).any() and not torch.isnan(mag).any() and not torch.isnan(ph).any()      # every element was written
    Xo, mago, pho = ops.stft_forward(w, L, hop, win, window=wd, lengths=LENS)                             # the torch front end: same bits
    assert torch.equal(torch.view_as_real(Xo), X) and torch.equal(mago, mag) and torch.equal(pho, ph)
    only = ops.stft_forward(w, L, hop, win, window=wd, lengths=torch.tensor(LENS), want_complex=False, want_phase=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], mag)
    worst = 0.0
    for b, (n, (Tb, _)) in enumerate(zip(LENS, counts(hop))):
        Xr = R.stft(E.clips()[b:b + 1, :n], n, hop, win, window)
        for ratio in (R.spec_ratio(torch.view_as_complex(X[b:b + 1, :, :Tb].contiguous()), Xr), R.spec_ratio(mag[b:b + 1, :, :Tb], Xr.abs())):
            worst = max(worst, ratio)
            assert ratio <= 1, (geom, fb, n, ratio)
        Xa, maga, pha = ops.stft_forward(w[b:b + 1, :n].contiguous(), n, hop, win, window=wd)             # the clip alone
        assert torch.equal(torch.view_as_real(Xa), X[b:b + 1, :, :Tb]) and torch.equal(maga, mag[b:b + 1, :, :Tb]), (geom, fb, n)
        assert torch.equal(pha, ph[b:b + 1, :, :Tb]), (geom, fb, n)
        assert (X[b, :, Tb:] == 0).all() and (mag[b, :, Tb:] == 0).all() and (ph[b, :, Tb:] == 0).all(), (geom, fb, n)
    print(f"ragged forward {geom} FB={fb}: worst error / bound {worst:.3f}")
    for junk in (float("nan"), 1e30):                                                                   # what lies past a clip is not read
        wj = w.clone()
        for b, n in enumerate(LENS):
            wj[b, n:] = junk
        Xj, magj, phj = forward_raw(wj, lens_d, hop, win, wd, T)
        assert torch.equal(Xj, X) and torch.equal(magj, mag) and torch.equal(phj, ph), (geom, fb, junk)


def inverse_raw(X, mask, lens_d, mode, hop, win, wd):
    w_in, w_out = (torch.full((B, L), float("nan"), device=X.device) for _ in range(2))
    rc = _lib.lib().advh_istft_masked_c64_ragged(X.data_ptr(), mask.data_ptr(), mask.shape[1], mask.shape[2], mode, w_in.data_ptr(),
                                                 w_out.data_ptr(), L, lens_d.data_ptr(), B, X.shape[2], L, hop, win,
                                                 None if wd is None else wd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "advh_istft_masked_c64_ragged")
    return w_in, w_out


@pytest.mark.parametrize("domain", ["log1p", "linear"])
@pytest.mark.parametrize("geom,fb", CASES, ids=[f"{g}-fb{fb}" for g, fb in CASES])
def test_inverse(gpu_device, frames_per_workgroup, geom, fb, domain):
    _lib.init()
    frames_per_workgroup(fb)
    hop, win, window, wd = geometry(geom, gpu_device)
    T = 1 + L // hop
    Wd = 4 * (T // 4)
    w = E.clips().to(gpu_device)
    lens_d = torch.tensor(LENS, dtype=torch.int32, device=gpu_device)
    Xc, _, _ = ops.stft_forward(w, L, hop, win, window=wd, lengths=LENS, want_mag=False, want_phase=False)
    X = torch.view_as_real(Xc).contiguous()
    mask = torch.rand(B, 512, Wd, generator=torch.Generator().manual_seed(11))
    mask[0, :100, :3], mask[1, 256:, :] = 0.0, 1.0                                                      # exact zeros and ones included
    mask = mask.to(gpu_device)
    mode = {"linear": 1, "log1p": 2}[domain]
    w_in, w_out = inverse_raw(X, mask, lens_d, mode, hop, win, wd)
    assert not torch.isnan(w_in).any() and not torch.isnan(w_out).any()
    o_in, o_out = ops.istft_masked_c64(Xc, mask, L, domain, hop=hop, win=win, window=wd, lengths=LENS)
    assert torch.equal(o_in, w_in) and torch.equal(o_out, w_out)
    assert torch.equal(ops.istft_masked_c64(Xc, mask, L, domain, want_in=False, hop=hop, win=win, window=wd, lengths=LENS)[1], w_out)
    assert torch.equal(ops.istft_masked_c64(Xc, mask, L, domain, want_out=False, hop=hop, win=win, window=wd, lengths=LENS)[0], w_in)
    w64 = R.window_of(win, window)
    worst = 0.0
    for b, (n, (Tb, Wb)) in enumerate(zip(LENS, counts(hop))):
        Xb, mb = Xc[b:b + 1, :, :Tb].contiguous(), mask[b:b + 1, :, :Wb].contiguous()
        for which, got in ((0, w_in), (1, w_out)):
            spec64 = R.apply_mask(mb.cpu(), Xb.cpu().to(torch.complex128), domain, which)
            ref = torch.istft(spec64, n_fft=1024, hop_length=hop, win_length=win, window=w64, length=n)
            ratio = R.wave_ratio(got[b:b + 1, :n], ref)
            worst = max(worst, ratio)
            assert ratio <= 1, (geom, fb, domain, n, which, ratio)
        a_in, a_out = ops.istft_masked_c64(Xb, mb, n, domain, hop=hop, win=win, window=wd)               # the cropped clip alone
        assert torch.equal(a_in, w_in[b:b + 1, :n]) and torch.equal(a_out, w_out[b:b + 1, :n]), (geom, fb, domain, n)
        assert (w_in[b, n:] == 0).all() and (w_out[b, n:] == 0).all(), (geom, fb, domain, n)
    print(f"ragged inverse {geom} FB={fb} {domain}: worst error / bound {worst:.3f}")
    Xj, mj = X.clone(), mask.clone()
    for b, (Tb, Wb) in enumerate(counts(hop)):
        Xj[b, :, Tb:] = float("nan")
        mj[b, :, Wb:] = float("nan")
    j_in, j_out = inverse_raw(Xj, mj, lens_d, mode, hop, win, wd)
    assert torch.equal(j_in, w_in) and torch.equal(j_out, w_out), (geom, fb, domain)


def test_refusals_happen_on_the_host(gpu_device):
    w = E.clips()[:2].to(gpu_device)
    for bad, msg in (([8000, 965], "clip 1 has 965"), ([8001, 8000], r"lengths\[0\] = 8001 exceeds"), ([8000], "1 entries for a batch of 2"),
                     ([8000.0, 966], "not an integer"), (torch.tensor([8000.0, 966.0]), "integer tensor")):
        with pytest.raises(ValueError, match=msg):
            ops.stft_forward(w, L, lengths=bad)
    with pytest.raises(ValueError, match="columns"):
        ops.stft_forward(w[:, :7000].contiguous(), L, lengths=[7000, 966])
    Xc = torch.zeros(2, 513, 25, dtype=torch.complex64, device=gpu_device)
    with pytest.raises(ValueError, match="clip 0 has 512"):
        ops.istft_masked_c64(Xc, torch.zeros(2, 512, 24, device=gpu_device), L, lengths=[512, 8000])
