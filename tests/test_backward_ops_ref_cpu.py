"""CPU-only: pins tests/backward_ops_ref.py (the fp64 restatement behind tests/test_gpu_backward_kernels.py) against
``torch.autograd`` in float64, at the awkward sizes too, and checks on the CPU the facts that two GPU cases rest on: the
offset-row LayerNorm case separates a two-pass from a one-pass variance, and the inputs of the linearity case keep every
rounded quantity inside its format's full-precision range."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_kernel_cases as K
import backward_ops_ref as BR

TOL = 1e-12           # both sides are float64: rounding only


def rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


@pytest.mark.parametrize("M,C", [(37, 768), (1, 4), (1, 2048), (5, 120)])
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("extras", [False, True])
def test_layernorm_bwd_matches_autograd(M, C, gelu, extras):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    dy, z, add = (torch.randn(M, C, generator=g, dtype=torch.float64) for _ in range(3))
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        y = F.layer_norm(xr, (C,), gamma, beta, 1e-5)
        if gelu:
            y = F.gelu(y)
        (ref,) = torch.autograd.grad(y, xr, dy)
        if extras:
            zr = z.clone().requires_grad_(True)
            (gz,) = torch.autograd.grad(F.gelu(zr).sum(), zr)
            ref = ref * gz + add
    got = BR.layernorm_bwd(x, dy, gamma, beta, 1e-5, gelu, z if extras else None, add if extras else None)
    assert rel(got, ref) <= TOL


@pytest.mark.parametrize("T,dm", [(1, 8), (17, 8), (16, 64), (65, 120), (5, 32)])
def test_attention_bwd_matches_autograd(T, dm):
    g = torch.Generator().manual_seed(T + dm)
    B, heads = 2, 3
    q, k, v, dO = (torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) for _ in range(4))
    with torch.enable_grad():
        qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
        s = qr @ kr.transpose(-1, -2) / math.sqrt(dm)
        s.retain_grad()
        p = torch.softmax(s, -1)
        (p @ vr).backward(dO)
    dq, dk, dv, P, dS = BR.attention_bwd(q, k, v, dO)
    for got, ref in ((dq, qr.grad), (dk, kr.grad), (dv, vr.grad), (P, p.detach())):
        assert rel(got, ref) <= TOL
    if T > 1:                                    # one key: dS is identically zero
        assert rel(dS, s.grad / math.sqrt(dm)) <= TOL           # dS carries the 1 / sqrt(d) of the scores, as in the kernels
    else:
        assert dS.abs().max().item() <= TOL and dq.abs().max().item() <= TOL and torch.equal(dv, dO)


def test_rows_and_heads_are_inverse():
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(3 * 5, 3 * 2 * 8, generator=g)
    assert torch.equal(BR.rows_of(*BR.heads_of(rows, 3, 5, 2, 8)), rows)
    q, k, v = BR.heads_of(rows, 3, 5, 2, 8)
    assert torch.equal(k[1, 1, 4], rows[1 * 5 + 4, 16 + 8:16 + 16])


def test_f16_model_rounds_only_where_stated():
    """With its rounding off the model IS the plain restatement; with it on, fp16 inputs give fp16-representable outputs that sit
    within the fp16 budget of the plain ones (P, dS: 2^-11 of each term; output: 2^-11)."""
    g = torch.Generator().manual_seed(4)
    q, k, v, dO = (torch.randn(2, 2, 33, 24, generator=g).half().double() for _ in range(4))
    plain = BR.attention_bwd(q, k, v, dO)
    off = BR.attention_bwd_f16_model(q, k, v, dO, rounding=False)
    on = BR.attention_bwd_f16_model(q, k, v, dO)
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(off[n], plain[i]) and torch.equal(off[n], off[n + "_pre"])
        assert torch.equal(on[n], on[n].half().double())
    P, dS = plain[3].abs(), plain[4].abs()
    budget = {"dq": dS @ k.abs(), "dk": dS.transpose(-1, -2) @ q.abs(), "dv": P.transpose(-1, -2) @ dO.abs()}
    for i, n in enumerate(("dq", "dk", "dv")):
        bound = 2.0 ** -11 * (budget[n] + plain[i].abs()) * (1 + 2.0 ** -6)
        assert ((on[n] - plain[i]).abs() <= bound).all()
        assert (on[n] != plain[i]).any()                        # the rounding is really on
    # the fp32 restatement of the model agrees with it to fp32 accuracy (plus the odd dS / P that rounds the other way)
    for a, b in zip(K.attention_bwd_f16_np32(q, k, v, dO), (on["dq_pre"], on["dk_pre"], on["dv_pre"])):
        assert rel(a, b) < 1e-3


def test_offset_rows_separate_one_pass_from_two_pass():
    """The offset-row case of the GPU suite: its bar (4x the error of an fp32 two-pass restatement) must be one that an fp32
    one-pass variance misses, or the case proves nothing."""
    x, dy, gamma = K.offset_rows()
    ref = BR.layernorm_bwd(x, dy, gamma, None, K.LN_EPS, 0)
    two = (K.ln_dx_np32(x, dy, gamma, K.LN_EPS, one_pass=False).double() - ref).abs().max().item()
    one = (K.ln_dx_np32(x, dy, gamma, K.LN_EPS, one_pass=True).double() - ref).abs().max().item()
    print(f"offset rows: fp32 two-pass err {two:.3e}, one-pass err {one:.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert two > 0 and one > 4 * two


def test_linearity_inputs_stay_in_range():
    lo, hi = K.linear_precondition(*K.linear_inputs())
    print(f"linearity inputs: magnitudes of dS * scale and the outputs over the scaled launches in [{lo:.3e}, {hi:.3e}]")
    assert K.LINEAR_RANGE[0] <= lo and hi <= K.LINEAR_RANGE[1]


def test_peaked_inputs_are_peaked():
    for fmt in ("f16", "split"):
        T, heads, dm, B = K.PEAKED_SHAPE
        qkv, dctx = K.peaked_inputs(fmt)
        q, k, v = BR.heads_of(qkv, B, T, heads, dm)
        s = q @ k.transpose(-1, -2) / math.sqrt(dm)
        P = torch.softmax(s, -1)
        assert P.max(-1).values.min().item() > 0.999
        assert (s.max(-1).values - s.min(-1).values).min().item() > 40


def test_embedder_grad_names_the_f16_limit():
    """The f16 chain cannot differentiate head dims above 64 beyond 208 frames (advh_attention_bwd_f16, include/addvisor_hip.h): the
    error says so before anything is launched, instead of a bare ADVH_EUNSUPPORTED."""
    import types

    from addvisor_hip import _lib
    from addvisor_hip.embedder_grad import F16_WIDE_HEAD_MAX_T, EmbedderGrad
    assert F16_WIDE_HEAD_MAX_T == 208 and K.refused_f16(209, 72) and not K.refused_f16(208, 128) and not K.refused_f16(256, 64)
    with pytest.raises(_lib.AdvhError, match=r"ADVH_EUNSUPPORTED: head dim 120 > 64 .* T <= 208 frames"):
        EmbedderGrad._att_bwd(types.SimpleNamespace(split=False), None, None, None, 1, 209, 240, 2, None)
