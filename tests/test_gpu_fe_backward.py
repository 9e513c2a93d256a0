"""The input-gradient chain below the encoder -- positional-conv backward, feature-projection GEMM and LayerNorm backward with
``remap``, the six ``plan_conv1d_dgrad`` GEMMs, the GroupNorm / front-end backward, ``g_plan`` and ``advh_wave_bwd`` as
``EmbedderGrad.backward`` composes them -- against float64 at every clip-length class (tests/fe_backward_ref.py; held on the CPU by
tests/test_fe_backward_ref_cpu.py).  The kernels underneath have suites of their own; this one tests the planner's launches on the
buffers the workspace lays out, and the composition.

a. ``plan_conv1d_dgrad`` launched as ``backward`` launches it, against ``gemm_desc_ref.bound``; rows past a clip's reach +0, guard
   and slack rows of the output untouched.
b. ``forward(to_layer=0)`` + ``backward(from_layer=0, layer_seed=S)`` against ``lower_chain_vjp`` at every length of
   ``fe_backward_ref.LENGTHS``, three clips, both tiny variants, both precisions: over the batch and, per clip, over the first and
   the last 400 samples alone (each normalised by its own max |ref|), so that a cross-clip leak or a wrong last frame cannot hide
   under the clip's largest gradient.
c. the same chain across calls of one ``EmbedderGrad``: other lengths and seeds in between, bit-identical repeats, after a full
   forward + backward; the filler, guard and slack rows of every ``dz`` level still zero afterwards.
d. the whole chain (``test_gpu_backward.grad_case``) at one frame, L = 400 and L = 645, three clips.
e. a clip shorter than the receptive field is refused before anything is allocated.

``LOSS_SCALE`` = 256: the largest gradient at any feature-encoder level of the fp64 reference is about 21 for these seeds (unit
normal seeds at every element of hidden_states[0]), so 256 keeps the fp16-range planes a factor 12 below 65504 where the default
4096 -- sized for the logit's gradient -- would leave the range.

Measured on an MI355X against the fp64 reference, worst max |dx - ref| / max |ref| over the table of b (batch, head and tail
windows of every clip) per precision, and the tolerance ``fe_backward_ref.TOL`` set from it (four times the worst, rounded up to
one significant digit, never above the whole chain's tolerance in tests/test_gpu_backward.py):
  f32  2.096e-6  layer_preln, L = 16000, tail window   -> 8.4e-6 -> tol 9e-6  (ceiling 1e-4);  lowest cosine 1.000000000
  f16  5.153e-3  layer_preln, L = 645, head window     -> 2.06e-2 -> tol 3e-2 (the ceiling);   lowest cosine 0.999996767 (same case)
The steps of c stay below the table's worst (f32 1.7e-6, f16 3.6e-3).  hidden_states[0]: f32 at most 4.5e-6 (bar 1e-4), f16 at
most 1.15e-2 max / 1.12e-3 mean (bars 3e-2 / 3e-3).  a: worst |err| / bound 0.967 (fp16, the half-ulp of the store), 0.032
(split), with ``dact_src`` 0.012 / 0.003.  d: f32 9.3e-7 ... 1.7e-6, f16 1.7e-3 ... 3.7e-3 of max |ref|.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fe_backward_ref as FR
import gemm_desc_ref as R
import test_fe_backward_ref_cpu as C
from addvisor_hip import _lib, synthetic as syn
from addvisor_hip.embedder import FE_SLACK_ROWS, HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, plan_conv1d_dgrad
from test_gpu_backward import TOL as CHAIN_TOL, grad_case
from test_gpu_embedder import TOL_HID_MAX, TOL_HID_MEAN
from test_gpu_split import TOL_HID

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LOSS_SCALE = 256.0
PRECISIONS = ("f32", "f16")
SENTINEL = 3.0


def bits(t):
    return t.contiguous().view(torch.int16).numpy()


# ------------------------------------------------------------------------------------------------ a. the planner's launches
DGRAD_ROWS = [(B, L_out, P_out) for B in (1, 3) for L_out, P_out in C.ROWS] + [(3, 99, 100)]       # the last: more than one M tile


@pytest.mark.parametrize("dact", [False, True], ids=["plain", "dact"])
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
@pytest.mark.parametrize("Cout,Cin", C.CHANNELS[:2])
@pytest.mark.parametrize("k,s", C.KS)
def test_dgrad_launches_meet_the_replay(gpu_device, k, s, Cout, Cin, split, dact):
    _lib.init()
    dev = gpu_device
    worst = 0.0
    for B, L_out, P_out in DGRAD_ROWS:
        c = C.dgrad_case(k, s, Cout, Cin, B, L_out, P_out, split, 0.75 if dact else None, seed=L_out)
        rep, d, planes = C.replay_dgrad(c.plan, c.nt, c.dz_buf, Cout, c.out_buf, Cin, c.dact_buf)      # audited on the host first
        ref, mask = rep.out["out_h"]
        plan, nt = plan_conv1d_dgrad(B, P_out, c.w, s, dev, split=split)
        assert plan.desc.N == 64 and plan.BN == 64 and (B * P_out > 256) == (P_out == 100)             # 256-row tiles: two only for the last
        dz = c.dz_buf.to(dev)
        out = torch.full_like(c.out_buf, SENTINEL).to(dev)           # guard row in front, slack rows behind: all sentinel
        src = None if c.dact_buf is None else c.dact_buf.to(dev)
        body = lambda t, Cn: t[..., Cn:]
        plan.run(dz if nt == 2 else body(dz, Cout), out_h=body(out, Cin), dact_src=None if src is None else body(src, Cin))
        torch.cuda.synchronize()
        got = out.cpu().reshape(-1, c.out_buf.shape[-1])             # [planes, pitch]
        init = bits(torch.full((1,), SENTINEL, dtype=torch.float16))[0]
        n = B * c.P_in * Cin
        assert mask[:n].all() and not mask[n:].any()
        past = np.zeros(n, dtype=bool).reshape(B, c.P_in, Cin)
        past[:, c.reach:] = True
        for pl in range(got.shape[0]):
            gb = bits(got[pl])
            assert (gb[:Cin] == init).all(), "the guard row in front of the output changed"
            assert (gb[Cin + n:] == init).all(), "a slack row behind the output changed"
            assert not gb[Cin:Cin + n][past.reshape(-1)].any(), "a row past a clip's reach is not +0"
        val = got[0, Cin:].double().numpy() + (got[1, Cin:].double().numpy() * 2.0 ** -11 if split else 0.0)
        assert np.isfinite(val[mask]).all()
        err, bnd = np.abs(val - ref)[mask], R.bound(d, rep, "out_h")[mask]
        ratio = float((err / np.maximum(bnd, 1e-300)).max())
        worst = max(worst, ratio)
        assert (err <= bnd).all(), f"B={B} L_out={L_out} P_out={P_out}: |err| / bound = {ratio:.3f}"
    print(f"FEBWD dgrad k={k} s={s} {Cout}->{Cin} {'split' if split else 'f16'} dact={dact}: worst |err|/bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ b. the chain against fp64
@pytest.fixture(scope="module")
def chains(gpu_device):
    """One ``EmbedderGrad`` per (variant, precision), built on first use and shared by the tests of this file."""
    made = {}

    def get(variant, precision):
        if (variant, precision) not in made:
            cfg, sd = FR.model(variant)
            coef, icpt = syn.logreg_weights(cfg.hidden_size)
            made[variant, precision] = EmbedderGrad(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision=precision))
        return made[variant, precision]
    return get


def run_lower(eg, waves, S):
    h = eg.forward(waves.to(eg.dev), to_layer=0)
    dx = eg.backward(LOSS_SCALE, from_layer=0, layer_seed=S.to(eg.dev))
    return h.cpu(), dx.cpu()


def check_forward(h, ref_h, precision, tag):
    err = (h.double() - ref_h).abs()
    print(f"FEBWD {tag} hidden_states[0]: max err {err.max():.3e} mean {err.mean():.3e} (|ref| max {ref_h.abs().max():.2f})")
    if precision == "f16":
        assert err.max().item() <= TOL_HID_MAX and err.mean().item() <= TOL_HID_MEAN, tag
    else:
        assert err.max().item() <= TOL_HID, tag


def check_dx(dx, ref, precision, tag):
    """Every figure is printed before anything is asserted."""
    assert tuple(dx.shape) == tuple(ref.shape)
    finite = bool(torch.isfinite(dx).all())
    r = FR.window_ratios(dx, ref) if finite else dict(all=float("nan"), head=float("nan"), tail=float("nan"))
    cos = F.cosine_similarity(dx.double().flatten(), ref.flatten(), dim=0).item()
    print(f"FEBWD {tag} dx: all {r['all']:.3e} head {r['head']:.3e} tail {r['tail']:.3e} cosine {cos:.9f} (|ref| max {ref.abs().max():.3e})")
    assert finite, tag
    tol = FR.TOL[precision]
    assert tol <= FR.CEILING[precision]
    assert r["all"] < tol and r["head"] < tol and r["tail"] < tol, (tag, r)
    assert cos > CHAIN_TOL[precision][1], tag


@pytest.mark.parametrize("L", list(FR.LENGTHS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", FR.VARIANTS)
def test_lower_chain_against_fp64(chains, variant, precision, L):
    eg = chains(variant, precision)
    assert eg.precision == precision
    cfg, _ = FR.model(variant)
    waves, S, ref_h, ref_dx = FR.reference(variant, L)
    h, dx = run_lower(eg, waves, S)
    f, r = eg._workspace(FR.B_CLIPS, L)["f"], FR.rows(L, cfg)
    assert (f["Ls"], f["P"], f["T"]) == (r.Ls, r.P, r.T)
    tag = f"{variant} {precision} L={L}"
    check_forward(h, ref_h, precision, tag)
    check_dx(dx, ref_dx, precision, tag)


# ------------------------------------------------------------------------------------------------ c. state between calls
def unwritten_rows_are_zero(eg, L):
    """Guard row, the filler rows of every clip and the slack rows of every ``dz`` level (every plane): still zero."""
    w = eg._workspace(FR.B_CLIPS, L)
    Ls, P, Cd = w["f"]["Ls"], w["f"]["P"], eg.cfg.conv_dim
    for i, t in enumerate(w["dz"]):
        flat = t.cpu().reshape(-1, t.shape[-1])
        for pl in flat:
            body = pl[Cd[i]:Cd[i] * (1 + FR.B_CLIPS * P[i])].view(FR.B_CLIPS, P[i], Cd[i])
            assert not pl[:Cd[i]].any(), f"dz[{i}]: guard row"
            assert not body[:, Ls[i]:].any(), f"dz[{i}]: filler rows"
            assert not pl[Cd[i] * (1 + FR.B_CLIPS * P[i]):].any(), f"dz[{i}]: slack rows"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", FR.VARIANTS)
def test_state_between_calls(chains, variant, precision):
    eg = chains(variant, precision)
    tag = f"{variant} {precision} state"
    step = lambda n, L, clip_seed, seed: (n,) + FR.reference(variant, L, clip_seed=clip_seed, seed=seed)
    for n, waves, S, ref_h, ref_dx in (step(1, 645, 5, 11), step(2, 640, 6, 12), step(3, 645, 6, 13)):
        h, dx = run_lower(eg, waves, S)
        check_forward(h, ref_h, precision, f"{tag} step {n}")
        check_dx(dx, ref_dx, precision, f"{tag} step {n}")
    h4 = eg.forward(waves.to(eg.dev), to_layer=0).cpu()              # 4: the same call once more; the backward only reads the saves
    w = eg._workspace(FR.B_CLIPS, 645)
    saves = [t for key in ("y", "z") for t in w[key] if t is not None] + [w["feat"], w["pc"], w["h1"], w["x"][0]]
    before = [t.clone() for t in saves]
    dx4 = eg.backward(LOSS_SCALE, from_layer=0, layer_seed=S.to(eg.dev)).cpu()
    assert torch.equal(h4, h) and torch.equal(dx4, dx)
    assert all(torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)) for a, b in zip(saves, before))
    wd = waves.to(eg.dev)
    eg.forward(wd)                                                   # 5: a whole forward + backward in between,
    eg.backward()
    eg.forward(wd)                                                   #    then the lower chain after a whole forward
    dx5 = eg.backward(LOSS_SCALE, from_layer=0, layer_seed=S.to(eg.dev)).cpu()
    check_dx(dx5, ref_dx, precision, f"{tag} step 5")
    assert torch.equal(dx5, dx)                                      # the saves below layer 0 are the same, and read-only
    for L in (645, 640):
        unwritten_rows_are_zero(eg, L)


# ------------------------------------------------------------------------------------------------ d. the whole chain, one frame
@pytest.mark.parametrize("L", [400, 645])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", FR.VARIANTS)
def test_whole_chain_at_one_frame(gpu_device, variant, precision, L):
    """``T = 1`` through the encoder, the attention backward and the pooling, at the tolerances of tests/test_gpu_backward.py."""
    cfg, _ = FR.model(variant)
    assert cfg.frames(L) == 1
    grad_case(cfg, syn.make_clips(FR.B_CLIPS, L, seed=FR.CLIP_SEED), gpu_device, 3e-2, precision)


# ------------------------------------------------------------------------------------------------ e. too-short clips
@pytest.mark.parametrize("precision", PRECISIONS)
def test_short_clip_is_refused(chains, precision):
    eg = chains("group_postln", precision)
    emb = eg.emb
    torch.cuda.synchronize()
    keys, gkeys, mem = set(emb._ws), set(eg._ws), torch.cuda.memory_allocated()
    msg = "shortest supported length is 400 samples"
    with pytest.raises(ValueError, match=msg):
        emb._workspace(1, 399)
    with pytest.raises(ValueError, match=msg):
        eg.forward(torch.zeros(1, 399))
    short = torch.zeros(1, 399, device=eg.dev)
    mem += short.numel() * 4
    with pytest.raises(ValueError, match=msg):
        eg.forward(short)
    with pytest.raises(ValueError, match=msg):
        emb.forward(short)
    assert set(emb._ws) == keys and set(eg._ws) == gkeys             # nothing planned,
    assert torch.cuda.memory_allocated() <= mem + 512                # nothing allocated (the clip itself, rounded up)
    emb._workspace(1, 400)                                           # and the shortest supported length is accepted
