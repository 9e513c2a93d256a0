"""tests/vocoder_ops_ref.py is the right operation: each fp64 helper equals the matching ``torch.nn.functional`` call in fp64, and the
generator composed from them equals oracle/hifigan_ref.py run in fp64, in both padding modes and with replicated mel frames.  No GPU.

Bound: both sides are fp64 sums of at most 11 * 128 products of O(1) values in different orders -- 1e-12 absolute on values of O(1)
(the waveform lies in [-1, 1])."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_ops_ref as R
from addvisor_hip import synthetic as syn
from oracle import hifigan_ref

TOL = 1e-12


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def cl(x):
    """[B, C, T] <-> [B, T, C]"""
    return x.transpose(1, 2)


@pytest.mark.parametrize("Cin,Cout,k,d,T", [(16, 24, 7, 1, 9), (8, 8, 11, 5, 60), (8, 8, 3, 3, 1), (8, 16, 11, 5, 5)])
def test_conv1d_same_matches_torch(Cin, Cout, k, d, T):
    g = torch.Generator().manual_seed(k * d + T)
    x, w, b = rnd(g, 3, T, Cin), rnd(g, Cout, Cin, k), rnd(g, Cout)
    pad = (k - 1) * d // 2
    ref = cl(F.conv1d(cl(x), w, b, padding=pad, dilation=d))
    assert (R.conv1d_same(x, w, b, d) - ref).abs().max().item() <= TOL
    assert (R.conv1d_same(x.float(), w.float(), b.float(), d).dtype == torch.float64)
    # a padded map whose halo is NOT zero: the taps read it
    halo = 32
    m = rnd(g, 3, T + 2 * halo, Cin)
    m[:, halo:halo + T] = x
    ref = cl(F.conv1d(cl(m[:, halo - pad:halo + T + pad]), w, b, dilation=d))
    got = R.conv1d_same(x, w, b, d, padded=m)
    assert tuple(got.shape) == (3, T, Cout) and (got - ref).abs().max().item() <= TOL
    if T > pad:                                                  # torch's reflect padding needs pad < T
        ref = cl(F.conv1d(F.pad(cl(x), (pad, pad), mode="reflect"), w, b, dilation=d))
        z = torch.zeros(3, T + 2 * halo, Cin, dtype=torch.float64)
        z[:, halo:halo + T] = x
        assert (R.conv1d_same(x, w, b, d, padded=R.halo_fill(z, T, halo, 1)) - ref).abs().max().item() <= TOL


@pytest.mark.parametrize("Cin,Cout,r,T", [(16, 8, 8, 5), (8, 4, 2, 1), (8, 8, 2, 37)])
def test_conv_transpose1d_matches_torch(Cin, Cout, r, T):
    g = torch.Generator().manual_seed(r + T)
    x, w, b = rnd(g, 2, T, Cin), rnd(g, Cin, Cout, 2 * r), rnd(g, Cout)
    ref = cl(F.conv_transpose1d(cl(x), w, b, stride=r, padding=r // 2))
    got = R.conv_transpose1d(x, w, b, r)
    assert tuple(got.shape) == (2, T * r, Cout) and (got - ref).abs().max().item() <= TOL


def test_resblock_step_mix_and_post_match_torch():
    g = torch.Generator().manual_seed(7)
    C, k, d, T = 8, 7, 3, 40
    x = rnd(g, 2, T, C)
    w1, b1, w2, b2 = rnd(g, C, C, k) * 0.2, rnd(g, C), rnd(g, C, C, k) * 0.2, rnd(g, C)
    t = F.leaky_relu(F.conv1d(F.leaky_relu(cl(x), 0.1), w1, b1, padding=(k - 1) * d // 2, dilation=d), 0.1)
    ref = cl(cl(x) + F.conv1d(t, w2, b2, padding=(k - 1) // 2))
    assert (R.resblock_step(x, w1, b1, w2, b2, d, 0.1) - ref).abs().max().item() <= TOL
    a, b, c = rnd(g, 2, T, C), rnd(g, 2, T, C), rnd(g, 2, T, C)
    assert (R.mrf_mix(a, b, c, 0.01) - F.leaky_relu((a + b + c) / 3)).abs().max().item() <= TOL
    assert (R.mrf_mix(a, b, c, 0.1) - F.leaky_relu((a + b + c) / 3, 0.1)).abs().max().item() <= TOL
    wp, bp = rnd(g, 1, C, k) * 0.1, 0.03
    xp = rnd(g, 2, T + k - 1, C)                                 # its first / last three rows are the (non-zero) padding
    y = F.conv1d(cl(xp), wp, torch.tensor([bp], dtype=torch.float64))[:, 0]
    wav, mass = R.conv_post(xp, wp, bp, k)
    assert tuple(wav.shape) == (2, T) and (wav - torch.tanh(y)).abs().max().item() <= TOL
    ref_mass = F.conv1d(cl(xp).abs(), wp.abs())[:, 0] + abs(bp)
    assert (mass - ref_mass).abs().max().item() <= TOL and (mass >= y.abs() - TOL).all()


@pytest.mark.parametrize("T", [1, 2, 5, 33, 40])
def test_halo_fill_and_pack_mel_match_torch(T):
    g = torch.Generator().manual_seed(T)
    halo, C = 32, 8
    m = torch.randn(2, T + 2 * halo, C, generator=g).half()
    z = R.halo_fill(m, T, halo, 0)
    assert z.dtype == torch.float16 and torch.equal(z[:, halo:halo + T], m[:, halo:halo + T])
    assert (z[:, :halo] == 0).all() and (z[:, halo + T:] == 0).all()
    f = R.halo_fill(m, T, halo, 1)
    n = min(halo, T - 1)
    want = cl(F.pad(cl(m[:, halo:halo + T]).float(), (n, n), mode="reflect")).half() if n else m[:, halo:halo + T]
    assert torch.equal(f[:, halo - n:halo + T + n], want)
    assert (f[:, :halo - n] == 0).all() and (f[:, halo + T + n:] == 0).all()
    mel = torch.randn(2, 16, T, generator=g)
    for pad in (0, 5):
        assert torch.equal(R.pack_mel(mel, pad), cl(F.pad(mel, (pad, pad), mode="replicate")))


@pytest.mark.parametrize("padding_mode", ["zeros", "reflect"])
@pytest.mark.parametrize("inference_padding", [0, 5])
def test_generator_matches_oracle_in_fp64(padding_mode, inference_padding):
    cfg = syn.hifigan_tiny_config()
    sd = syn.hifigan_weights(cfg)
    r = np.random.Generator(np.random.PCG64(9))
    mel = torch.from_numpy(r.normal(-4.0, 2.0, size=(2, cfg.in_channels, 9)).astype(np.float32))
    ref = hifigan_ref.generator(mel.double(), {k: v.double() for k, v in sd.items()}, cfg, padding_mode=padding_mode,
                                inference_padding=inference_padding)
    got = R.generator(mel, sd, cfg, padding_mode=padding_mode, inference_padding=inference_padding)
    assert got.dtype == ref.dtype == torch.float64 and got.shape == ref.shape == (2, 1, (9 + 2 * inference_padding) * cfg.hop)
    err = (got - ref).abs().max().item()
    print(f"fp64 generator ({padding_mode}, pad {inference_padding}) vs the oracle in fp64: {err:.2e}; ref absmax {ref.abs().max():.3f}")
    assert err <= TOL
