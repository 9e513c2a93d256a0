"""CPU-only checks behind tests/test_gpu_fe_backward.py: ``embedder_grad.plan_conv1d_dgrad`` means ``F.conv_transpose1d`` on the
buffers ``EmbedderGrad._workspace`` lays out (guard row, zero filler rows, slack rows), replayed in fp64 from its descriptor
(tests/gemm_desc_ref.py); the reference tells the planner's possible mistakes apart by more than the GPU tolerance; the length
table's claims; the fp64 chain reference against the same code in fp32; the head / tail windows of the GPU check carry signal."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fe_backward_ref as FR
import gemm_desc_ref as R
from addvisor_hip import gemm as G
from addvisor_hip.embedder import FE_SLACK_ROWS, HipEmbedder
from addvisor_hip.embedder_grad import plan_conv1d_dgrad

KS = [(3, 2), (2, 2)]
CHANNELS = [(32, 32), (64, 32), (24, 12)]              # (Cout, Cin): the unequal pairs catch a transposed weight block
ROWS = [(1, 2), (3, 6), (12, 13), (49, 50)]            # (L_out, P_out)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale


def gelu_grad(x):
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(torch.nn.functional.gelu(x).sum(), x)
    return g


def level_buffer(B, P, Cn, split, values=None, fill=0.0):
    """One feature-encoder level as ``EmbedderGrad._workspace`` allocates it: a guard row, ``[B][P][Cn]`` rows, ``FE_SLACK_ROWS``
    rows behind; fp16, or the plane pair.  ``values [B, L, Cn]`` go to rows ``< L`` of every clip, ``fill`` to the rows behind
    them; guard and slack rows stay zero.  Returns (buffer, the ``[B, P, Cn]`` view of its hi plane or of the buffer)."""
    n = (1 + B * P + FE_SLACK_ROWS) * Cn
    buf = torch.zeros((2, n) if split else (n,), dtype=torch.float16)
    body = buf[..., Cn:Cn + B * P * Cn].view(*buf.shape[:-1], B, P, Cn)
    if values is not None:
        L = values.shape[1]
        body[..., L:, :] = fill
        if split:
            body[:, :, :L] = FR.split_pair(values)
            if fill:
                body[1, :, L:] = 0.0
        else:
            body[:, :L] = values.half()
    return buf, body


def from_row(buf, Cn, row):
    """The flat memory behind the pointer ``EmbedderGrad.backward`` passes for ``buf`` from buffer row ``row`` on, and the plane
    pitch in elements: (flat numpy array, pitch)."""
    return buf.reshape(-1)[row * Cn:].numpy(), buf.shape[-1]


def replay_dgrad(plan, nt, dz_buf, Cout, out_buf, Cin, dact_buf=None, a0_row=None, W=None):
    """fp64 replay of the launch ``backward`` makes: ``A0`` = the dZ buffer (``nt == 2``: the guard row is row -1 of clip 0) or
    its body (``nt == 1``), ``out_h`` / ``dact_src`` = the bodies of the level below.  Returns (Replay, descriptor fields, planes)."""
    d = R.desc_fields(plan.desc)
    d.A0, d.A1, d.W, d.ktab, d.bias, d.out_h, d.resid, d.dact_src = True, False, True, True, False, True, False, dact_buf is not None
    a0, a_pitch = from_row(dz_buf, Cout, (0 if nt == 2 else 1) if a0_row is None else a0_row)
    out, o_pitch = from_row(out_buf, Cin, 1)
    bufs = {"A0": a0, "W": (plan.w if W is None else W).reshape(-1).numpy(), "ktab": plan.ktab_host}
    numel = {"A0": a0.size, "W": plan.w.numel(), "ktab": len(plan.ktab_host), "out_h": out.size}
    if dact_buf is not None:
        bufs["dact_src"], pitch = from_row(dact_buf, Cin, 1)
        assert pitch == o_pitch                                  # split outputs share one plane pitch (GemmPlan.run)
        numel["dact_src"] = bufs["dact_src"].size
    if plan.split:
        d.a_lo, d.o_lo = [a_pitch // 8, 0], o_pitch
    planes = {"out_h": o_pitch - Cin}                           # one plane, from the body's first row to the plane's end
    rep = R.replay(d, bufs, planes, plan.BN)
    R.audit(rep, numel)
    return rep, d, planes


def dgrad_case(k, s, Cout, Cin, B, L_out, P_out, split, dact=None, seed=0):
    """The planner on the CPU and the buffers of one case: ``dact``: None, or the value in the filler rows of ``dact_src``."""
    w = rnd(Cout, Cin, k, seed=seed, scale=(Cout * k) ** -0.5)
    plan, nt = plan_conv1d_dgrad(B, P_out, w, s, split=split)
    dz = rnd(B, L_out, Cout, seed=seed + 1)
    P_in, reach = s * P_out, s * (L_out - 1) + k
    dz_buf, _ = level_buffer(B, P_out, Cout, split, dz)
    out_buf, _ = level_buffer(B, P_in, Cin, split)
    zsrc = rnd(B, reach, Cin, seed=seed + 2, scale=1.5)
    dact_buf = None if dact is None else level_buffer(B, P_in, Cin, split, zsrc, fill=dact)[0]
    ref = FR.dgrad_ref(dz, w, s, split)
    if dact is not None:
        ref = ref * gelu_grad(FR.as_stored(zsrc, split))
    return SimpleNamespace(w=w, plan=plan, nt=nt, dz=dz, dz_buf=dz_buf, out_buf=out_buf, dact_buf=dact_buf, ref=ref, P_in=P_in,
                           reach=reach, B=B, Cout=Cout, Cin=Cin, s=s, k=k, L_out=L_out, P_out=P_out, split=split)


def test_operand_rounding_is_the_packers():
    x = rnd(5, 7, 8, scale=3.0)
    x[0, 0, :4] = torch.tensor([0.0, 2.0 ** -15, -2.0 ** -14, 1e-7])
    assert torch.equal(FR.split_pair(x), G.split_planes(x))
    assert torch.equal(FR.join_pair(FR.split_pair(x)).float(), G.join_planes(G.split_planes(x)))


@pytest.mark.parametrize("dact", [None, 0.0, 0.75], ids=["plain", "dact_zero_filler", "dact_finite_filler"])
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cout,Cin", CHANNELS)
@pytest.mark.parametrize("k,s", KS)
def test_planner_is_the_transposed_convolution(k, s, Cout, Cin, B, split, dact):
    for L_out, P_out in ROWS:
        c = dgrad_case(k, s, Cout, Cin, B, L_out, P_out, split, dact, seed=L_out)
        assert c.nt == -(-k // s) and c.reach <= c.P_in and P_out > L_out
        rep, d, planes = replay_dgrad(c.plan, c.nt, c.dz_buf, Cout, c.out_buf, Cin, c.dact_buf)
        val, mask = (torch.from_numpy(a) for a in rep.out["out_h"])
        n = B * c.P_in * Cin
        assert mask[:n].all() and not mask[n:].any()              # every row of the level is written, no slack row is
        v = val[:n].view(B, c.P_in, Cin)
        assert torch.allclose(v[:, :c.reach], c.ref, rtol=0, atol=1e-12)
        assert (v[:, c.reach:] == 0).all()                        # rows past a clip's reach: exactly zero
        # the guard row is read (nt == 2: row -1 of clip 0) and the furthest read ends with the last [B][P_out] row: inside
        # the buffer, the slack rows behind it untouched by this launch
        hi_plane = [r for r in rep.reads["A0"] if r[0] < c.dz_buf.shape[-1]]          # the lo plane starts one pitch behind the pointer
        assert hi_plane[0][0] == 0 and max(r[1] for r in hi_plane) == (c.nt - 1 + B * P_out) * Cout


def unpack_rows(plan):
    """The plan's packed weight as the logical ``[N, Ktot]`` matrix (the wide epilogue permutes its rows) and the inverse."""
    wp = plan.w.reshape(-1, plan.Kp)
    chan = G.packed_row_channel(wp.shape[0]) if plan.desc.wide else np.arange(wp.shape[0])
    keep = np.nonzero(chan < plan.desc.N)[0]
    logical = torch.zeros(plan.desc.N, plan.Kp, dtype=wp.dtype)
    logical[torch.from_numpy(chan[keep])] = wp[torch.from_numpy(keep)]

    def pack(m):
        out = torch.zeros_like(wp)
        out[torch.from_numpy(keep)] = m[torch.from_numpy(chan[keep])]
        return out
    return logical, pack


def test_unpack_rows_is_the_planners_matrix():
    c = dgrad_case(3, 2, 64, 32, 3, 12, 13, False)
    m, pack = unpack_rows(c.plan)
    assert torch.equal(pack(m), c.plan.w.reshape(-1, c.plan.Kp))
    # row phase * Cin + ci, column i * Cout + co holds W[co, ci, phase + s * (nt - 1 - i)]: the block is the tap, transposed
    assert torch.equal(m[32:64, 64:128], c.w[:, :, 1].t().half()) and not m[32:64, :64].any()          # tap 3 does not exist
    assert torch.equal(m[0:32, 0:64], c.w[:, :, 2].t().half()) and torch.equal(m[0:32, 64:128], c.w[:, :, 0].t().half())


def test_reference_tells_the_planners_mistakes_apart():
    """Each single mistake moves the replayed result away from ``dgrad_ref`` by more than the loosest tolerance the GPU suite
    holds the chain to (of max |ref|), so a planner or a workspace making it cannot pass."""
    tol = max(FR.TOL.values())
    c = dgrad_case(3, 2, 64, 32, 3, 12, 13, False)               # one filler row per clip: clip 1 reads it as its row -1
    Cout, Cin, B = c.Cout, c.Cin, c.B
    n = B * c.P_in * Cin
    mx = c.ref.abs().max().item()

    def result(**kw):
        rep, _, _ = replay_dgrad(c.plan, c.nt, kw.pop("dz_buf", c.dz_buf), Cout, c.out_buf, Cin, **kw)
        return torch.from_numpy(rep.out["out_h"][0])[:n].view(B, c.P_in, Cin)[:, :c.reach]

    assert (result() - c.ref).abs().max().item() <= 1e-12
    m, pack = unpack_rows(c.plan)
    taps = m.clone()                                             # taps not reversed: tap block i <-> nt - 1 - i
    taps[:, :Cout], taps[:, Cout:2 * Cout] = m[:, Cout:2 * Cout], m[:, :Cout]
    phases = torch.cat([m[Cin:], m[:Cin]])                       # the two output phases swapped
    leak_buf = c.dz_buf.clone()
    leak_buf[(1 + c.L_out) * Cout:(2 + c.L_out) * Cout] = 1.0    # clip 0's filler row: row -1 of clip 1
    got = {"taps_not_reversed": result(W=pack(taps)), "phases_swapped": result(W=pack(phases)),
           "a0_one_row_late": result(a0_row=1), "filler_row_not_zero": result(dz_buf=leak_buf)}
    for name, v in got.items():
        assert (v - c.ref).abs().max().item() / mx > tol, name
    leak = (got["filler_row_not_zero"] - c.ref).abs()
    assert leak[1, :2].max().item() / mx > tol and not leak[1, 2:].any() and not leak[2].any()     # it is clip 1's first rows that move


def test_length_table_claims():
    cfg, _ = FR.model("group_postln")
    assert cfg.conv_kernel == (10, 3, 3, 3, 3, 2, 2) and cfg.conv_stride == (5, 2, 2, 2, 2, 2, 2)
    emb = object.__new__(HipEmbedder)                            # _lengths / min_length need the configuration alone
    emb.cfg = cfg
    assert emb.min_length() == FR.SHORTEST == min(FR.LENGTHS)
    for L, claim in FR.LENGTHS.items():
        r = FR.rows(L, cfg)
        assert r.Ls == emb._lengths(L) and r.T == cfg.frames(L), L
        for i in range(len(r.P) - 1):
            assert r.P[i] == r.P[i + 1] * cfg.conv_stride[i + 1], L
        assert all(p > l for p, l in zip(r.P, r.Ls)), L         # a zero filler row per clip at every level
        assert any((r.P[-1] - 1) * (p // r.P[-1]) <= l for p, l in zip(r.P, r.Ls)), L          # and no smaller P has one
        have = dict(T=r.T, Ls=r.Ls, P=r.P, P0=r.P[0], tight=r.tight, left=[i for i, v in enumerate(r.left) if v], fill0=r.P[0] - r.Ls[0])
        for key, want in claim.items():
            if key != "why":
                assert have[key] == want, (L, key, have[key])
    assert FR.rows(719, cfg).T == 1 and FR.rows(720, cfg).T == 2
    # the classes the table exists for are all present
    tight = [FR.rows(L, cfg).tight for L in FR.LENGTHS]
    assert [] in tight and FR.ALL_LEVELS in tight and {FR.rows(L, cfg).T for L in FR.LENGTHS} == {1, 2, 12, 49}


def test_short_clip_is_refused_before_anything_is_built():
    cfg, _ = FR.model("group_postln")
    emb = object.__new__(HipEmbedder)
    emb.cfg, emb._ws, emb.dev, emb.sd = cfg, {}, None, {}        # no device, no weights: the refusal needs neither
    for L in (399, 10, 0):
        with pytest.raises(ValueError, match="shortest supported length is 400 samples"):
            emb._workspace(1, L)
    assert emb._ws == {}


@pytest.mark.parametrize("variant", FR.VARIANTS)
def test_fp64_chain_reference_against_fp32_and_windows(variant):
    """fp32 autograd of the same code agrees with the fp64 reference to 1e-5 of max |ref| at every length (measured: at most
    1.5e-6), and the first and the last 400 samples of every clip carry at least 0.1 of the clip's largest gradient (measured:
    at least 0.145), so the windowed checks of the GPU suite are not dominated by the middle of the clip."""
    for L in FR.LENGTHS:
        waves, S, h, dx = FR.reference(variant, L)
        cfg, sd = FR.model(variant)
        assert h.dtype == dx.dtype == torch.float64 and tuple(dx.shape) == (FR.B_CLIPS, L) and tuple(h.shape) == tuple(S.shape)
        h32, dx32 = FR.lower_chain_vjp(cfg, sd, waves, S, torch.float32)
        assert dx32.dtype == torch.float32
        assert (dx32.double() - dx).abs().max().item() <= 1e-5 * dx.abs().max().item(), L
        assert (h32.double() - h).abs().max().item() <= 1e-5 * h.abs().max().item(), L
        for b in range(FR.B_CLIPS):
            mx = dx[b].abs().max().item()
            assert math.isfinite(mx) and mx > 0
            assert dx[b, :FR.WINDOW].abs().max().item() >= 0.1 * mx, (L, b, "head")
            assert dx[b, -FR.WINDOW:].abs().max().item() >= 0.1 * mx, (L, b, "tail")
