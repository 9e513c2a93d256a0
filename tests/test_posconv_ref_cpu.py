"""CPU-only: tests/posconv_ref.py against fp64 torch and its autograd, its mirrors of the host arithmetic against the library,
the claims its case tables make, the conditions under which the bit-exact GPU test cannot hide a failure, and the truth table
of the selector that sends the positional convolution to the line tile."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posconv_ref as R
from addvisor_hip import _lib, embedder, gemm as G


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("Cg,G_,B,T,K", [(8, 2, 2, 5, 4), (16, 3, 2, 21, 16), (48, 2, 1, 17, 128)])
@torch.enable_grad()                                       # the GPU modules switch autograd off for the whole session on import
def test_refs_against_torch_autograd(Cg, G_, B, T, K):
    g = torch.Generator().manual_seed(T)
    H = Cg * G_
    h = torch.randn(B, T, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(H, Cg, K, generator=g, dtype=torch.float64) / (K * Cg) ** 0.5
    bias = torch.randn(H, generator=g, dtype=torch.float64)
    dh = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    z = F.conv1d(h.transpose(1, 2), w, bias, padding=K // 2, groups=G_)[:, :, :T].transpose(1, 2)
    y = h + F.gelu(z)
    ref, zr = R.forward_ref(h.detach(), w, bias, G_)
    assert (ref - y.detach()).abs().max().item() <= 1e-12 and (zr - z.detach()).abs().max().item() <= 1e-12
    (grad,) = torch.autograd.grad(y, h, dh)
    assert (R.backward_ref(dh, z.detach(), w, G_) - grad).abs().max().item() <= 1e-12
    # a residual that is not the convolution's operand
    other = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    assert (R.forward_ref(h.detach(), w, bias, G_, resid=other)[0] - (other + F.gelu(z.detach()))).abs().max().item() <= 1e-12


def test_tile_weights_and_gather_layout():
    """The weight stream element by element, and the same packing in ``embedder.pack_posconv_tile``."""
    Cg, G_, K = 48, 2, 128
    w = torch.randn(Cg * G_, Cg, K, generator=torch.Generator().manual_seed(3))
    wt = R.tile_weights(w, G_)
    assert wt.shape == (G_, K * Cg // 32, Cg, 32) and wt.dtype == torch.float16
    for g, s, n, j in ((0, 0, 0, 0), (1, 191, 47, 31), (0, 1, 5, 16), (1, 100, 17, 3)):           # 32 s + j = k * Cg + ci
        k, ci = divmod(32 * s + j, Cg)
        assert wt[g, s, n, j] == w[g * Cg + n, ci, k].half()
    assert torch.equal(embedder.pack_posconv_tile(w, G_), wt)
    x = torch.arange(2 * 3 * 16, dtype=torch.float32).view(2, 3, 16)
    xg = R.gather_ref(x, 2, 4, 1)
    assert xg.shape == (2, 2, 7, 8) and (xg[:, :, 0] == 0).all() and (xg[:, :, 4:] == 0).all()
    assert torch.equal(xg[1, 0, 2], x[0, 1, 8:])


# --------------------------------------------------------------------------------------------------------------- mirrors
def test_lds_bytes_mirror(lib):
    for Cg in (40, 48, 64):
        for T in range(1, 258):
            assert R.lds_bytes(Cg, T) == lib.advh_posconv_tile_lds_bytes(Cg, T), (Cg, T)
    assert R.lds_bytes(48, 0) == lib.advh_posconv_tile_lds_bytes(48, 0) == -1


def test_named_cases_have_the_properties_claimed():
    Cg, G_, B, T = R.NAMED[0]
    assert (Cg, G_, B, T) == R.SECOND_TRIP == (64, 16, 17, 130)
    assert G_ * B == 272 > R.grid(Cg, T, G_, B) == 256 and R.per_cu(Cg, T) == 1
    assert 256 // B == 15                                                     # block 0's second tile is in group 15, its first in group 0
    assert R.gather_items(Cg, G_, B, T, 128) == 1122816 > R.GATHER_TRIP == 1048576
    Cg, G_, B, T = R.NAMED[1]
    assert G_ * B == 528 > R.grid(Cg, T, G_, B) == 512 and R.per_cu(Cg, T) == 2
    assert (R.per_cu(64, 129), R.per_cu(64, 130), R.per_cu(48, 225), R.per_cu(48, 226)) == (2, 1, 2, 1)
    assert {(64, 2, 3, 129), (48, 2, 3, 225), (48, 2, 3, 226), (48, 1, 1, 1), (64, 16, 1, 256)} <= set(R.NAMED)
    assert all(R.lds_bytes(c[0], c[3]) > 0 for c in R.TILE_CASES + R.IDENTICAL_CASES)
    # no sweep case leaves its grid: the second trips are the named cases' alone
    assert all(G_ * B <= R.grid(Cg, T, G_, B) for Cg, G_, B, T in R.SWEEP)


def test_t_edges_reach_every_tile_count_and_pattern():
    assert len(R.T_EDGES) == 32
    assert {(T + 15) // 16 for T in R.T_EDGES} == set(range(1, 17))
    assert all({16 * (nt - 1) + 1, 16 * nt} <= set(R.T_EDGES) for nt in range(1, 17))
    every = {R.nj_of(T) for T in range(1, 257)}
    assert {R.nj_of(T) for T in R.T_EDGES} == every and len(every) == 16
    assert R.nj_of(1) == (1, 0, 0, 0) and R.nj_of(33) == (1, 1, 1, 0) and R.nj_of(256) == (4, 4, 4, 4)
    assert all(sum(R.nj_of(T)) == (T + 15) // 16 for T in range(1, 257))
    assert {c[:1] + c[3:] for c in R.SWEEP} == set(itertools.product(R.CG, R.T_EDGES))
    assert {c[3] for c in R.GEMM_CASES} == {1, 16, 17, 199, 256, 257, 300}
    assert {(c[0], c[4]) for c in R.GEMM_CASES} == {(32, 16), (48, 128), (64, 128), (120, 128)}


# ------------------------------------------------------------------------------------- the exact test's power
def test_gelu_fast_is_exact_from_six():
    """An fp32 emulation of gelu_fast returns exactly z (z >= 6) or -0 (z <= -6) for every integer |z| <= 2048: the p t e term of
    fast_erf is ~2e-9 there, below half an ulp of 1 with a factor of ~15 to spare over one-ulp rcp / exp2 error."""
    z = np.concatenate([np.arange(6, 2049), -np.arange(6, 2049)]).astype(np.float32)
    out = R.np_gelu_fast(z)
    assert np.array_equal(out, np.maximum(z, 0.0))
    assert np.signbit(out[z < 0]).all()
    # and the margin: the term that must vanish against 1, at the smallest argument
    u = 6.0 / 2.0 ** 0.5
    t = 1.0 / (1.0 + 0.3275911 * u)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    assert p * np.exp(-u * u) * 10 < 2.0 ** -25
    # inside (-6, 6) it is the approximation GELU_TOL[True] describes
    x = np.linspace(-6, 6, 4001)
    ref = R.gelu_erf(torch.from_numpy(x)).numpy()
    from gemm_desc_ref import GELU_TOL
    assert np.abs(R.np_gelu_fast(x).astype(np.float64) - ref).max() <= 6 * GELU_TOL[True]


FWD_INT = [c + (R.K_TILE,) for c in R.TILE_CASES] + list(R.GEMM_CASES)


@pytest.mark.parametrize("Cg,G_,B,T,K", FWD_INT, ids=lambda v: str(v))
def test_integer_forward_cases_are_exact_and_sharp(Cg, G_, B, T, K):
    """On the reference alone: every value stays an exact fp32 integer, and nearly every element is in the bit-exact class."""
    h, w, bias, ref, z = R.forward_case("int", False, Cg, G_, B, T, K)
    assert torch.equal(h.half().float(), h) and torch.equal(w.half().float(), w)
    assert h.abs().max() <= 2 and w.abs().max() <= 2 and bias.abs().max() <= 3
    assert torch.equal(z, z.round()) and z.abs().max().item() <= 2048
    assert ref.abs().max().item() < 2.0 ** 24
    big = z.abs() >= R.EXACT_Z
    share = big.double().mean().item()
    assert share >= (0.9 if T >= 16 else 0.6), share
    # the erf GELU itself is within 3 erfc(6 / sqrt 2) = 6e-9 of max(z, 0) there: far below half an fp32 ulp of any |z| >= 6
    assert (ref - R.exact_expected(h, z))[big].abs().max().item() <= 1e-8
    if (Cg, G_, B, T, K) in R.GEMM_CASES:                                       # the split operands are the same integers
        assert torch.equal(R.forward_case("int", True, Cg, G_, B, T, K)[3], ref)


@pytest.mark.parametrize("Cg,G_,B,T,K", R.GEMM_CASES, ids=lambda v: str(v))
def test_integer_backward_cases_are_exact(Cg, G_, B, T, K):
    dh, pcs, w, ref = R.backward_case("int", False, Cg, G_, B, T, K)
    assert set(dh.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(pcs.float().abs().unique().tolist()) <= {16.0, 24.0}
    g = R.gelu_grad(pcs.double())
    assert torch.equal(g.float(), (pcs > 0).float())                           # 1 or 0 to far below fp32
    assert ref.abs().max().item() < 2048                                       # integers fp16 holds exactly
    assert torch.equal(ref.float().double(), ref.round()) and ref.abs().max().item() > 8
    assert torch.equal(R.backward_case("int", True, Cg, G_, B, T, K)[3], ref)
    assert torch.equal(R.planes_value(R.backward_case("int", True, Cg, G_, B, T, K)[1]), pcs.double())


# -------------------------------------------------------------------------------------------------------- the selector
def test_posconv_tile_selector_truth_table(lib):
    """``POSCONV_TILE and not split and lds_bytes(Cg, T) > 0 and K == 128 and (Cg <= 48 or B <= 96)``."""
    assert embedder.POSCONV_TILE
    for split, K, Cg, T, B in itertools.product((False, True), (128, 16), (32, 48, 64, 120), (256, 257), (96, 97)):
        want = (not split) and K == 128 and Cg in (48, 64) and T <= 256 and (Cg == 48 or B <= 96)
        assert embedder.posconv_tile_selected(Cg, T, B, K, split) is want, (split, K, Cg, T, B)
    old = embedder.POSCONV_TILE
    try:
        embedder.POSCONV_TILE = False
        assert embedder.posconv_tile_selected(48, 199, 3, 128, False) is False
    finally:
        embedder.POSCONV_TILE = old


def test_plan_posconv_builds_the_models_descriptors():
    """The forward and the flipped plan against the constructions the embedder and its gradient chain used to spell out."""
    B, T, Cg, Gp, K = 2, 9, 16, 2, 16
    H, cc = Cg * Gp, Cg // 8
    g = torch.Generator().manual_seed(5)
    w, bias = torch.randn(H, Cg, K, generator=g), torch.randn(H, generator=g)
    src = [G.Source((T + K) * cc, 0, cc, 0, sZ=B * (T + K) * cc)]
    common = dict(M=B * T, N=Cg, ktab=np.arange(K * cc, dtype=np.int64), sources=src, Hg=1, Wg=T, window=(0, 1, 0, T),
                  halo_zero=False, out=(T * H, 0, H, 0), n_div=G.round_up(Cg, 4), o_sZ=Cg, nz=Gp)
    fwd = G.GemmPlan(w2=w.view(Gp, Cg, Cg, K).permute(0, 1, 3, 2).reshape(Gp, Cg, K * Cg), bias=bias, bias_sZ=Cg, act="gelu", **common)
    bwd = G.GemmPlan(w2=w.view(Gp, Cg, Cg, K).flip(3).permute(0, 2, 3, 1).reshape(Gp, Cg, K * Cg), **common)
    for old, new in ((fwd, embedder.plan_posconv(B, T, H, Gp, K, w, bias)), (bwd, embedder.plan_posconv(B, T, H, Gp, K, lambda: w, flip=True))):
        assert torch.equal(old.w, new.w) and np.array_equal(old.ktab_host, new.ktab_host) and old.tile == new.tile
        assert (old.bias is None) == (new.bias is None) and (old.bias is None or torch.equal(old.bias, new.bias))
        assert bytes(old.desc) == bytes(new.desc)
