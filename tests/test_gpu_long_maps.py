"""End to end: attention maps, attention rollout, gradient rollout and transformer LRP above 256 frames and on ragged batches
(``HipAttribution(long_clips=True, long_maps=True)``; csrc/attention_maps_long.hip), against the float64 restatements
``attention_rollout_ref.explain`` and ``lrp_ref.explain`` on the CPU.

Models: ``tiny_group`` (post-LN), ``tiny_layer`` (pre-LN) and ``head120`` of tests/test_gpu_long_clips.py, both precisions, one clip
at L = 82 320 (257 frames), 96 000 (299) and 164 240 (513; not head120), and the ragged batch of 513, 299, 124 and 1 frames.
L = 82 319 (256 frames) is the anchor: ``long_maps=True`` is bit-identical to the default chain there, on the launches this
feature leaves alone, and the default chain's own distance to float64 is what ``PARENT_BAR`` would be taken from.

Bars, the project's: f32 1e-4 of each tensor's own max|ref| and cosine > 0.999999; f16 3e-2 and 0.999 (tests/test_gpu_lrp.py,
tests/test_gpu_attention_rollout.py).  Every layer's Abar is judged on its own.  Every figure is printed before its assertion.

Measured on an MI355X, worst over the models and lengths above 256 frames: f32 A 3.7e-6, GA 3.3e-6, Abar 3.3e-6, R 1.4e-6, D 2.8e-6,
rollout relevances <= 1.4e-6, LRP R / rel 2.0e-6 / 2.1e-6, cosine 1.000000; f16 A 6.4e-3, GA 7.3e-3, Abar 7.9e-3 (cosine 0.99996),
R 2.5e-3, D 6.5e-3, LRP 5.4e-3 / 4.3e-3.  The default chain at L = 82 319 measures f32 <= 2.8e-6 and f16 <= 6.2e-3 (Abar cosine
0.99996) -- inside the bars, so ``PARENT_BAR`` is empty.  (head120, f16) has no gradient anchor: the fp16 whole-clip backward holds
head dims above 64 for T <= 208 frames, unchanged.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import attention_rollout_ref as AR
import lrp_ref as LR
import ragged_ref as RR
import test_gpu_long_clips as LC
from addvisor_hip import _lib
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}
# (model, precision, quantity) -> (error bar, cosine bar): twice what the default chain measures at L = 82 319 where that is above TOL
PARENT_BAR = {}
ANCHOR = 82319
LENGTHS = {"tiny_group": (82320, 96000, 164240), "tiny_layer": (82320, 96000, 164240), "head120": (82320, 96000)}
CASES = [(n, p, L) for n in LENGTHS for p in ("f32", "f16") for L in LENGTHS[n]]
RAGGED = LC.RAGGED
RULES = {"default": dict(), "all identity": dict(gelu_rule="identity"), "ln alone": dict(attention_rule=False),
         "attention alone": dict(ln_rule=False), "gelu alone": dict(ln_rule=False, attention_rule=False, gelu_rule="identity")}
FUSION = {"mean": "mean", "max": "max", "min": "min"}
NAN = float("nan")


def ref_model(name):
    cfg, sd, coef, icpt = LC.model(name)
    return sd, cfg, coef, icpt


@functools.lru_cache(maxsize=None)
def engine(name, precision, long_maps=True):
    return HipAttribution(LC.embedder(name, precision), long_clips=True, long_maps=long_maps)


@functools.lru_cache(maxsize=None)
def clip(L, n=None, b=0, batch=1):
    """Clip b of RR.clips(batch, L, 91), cropped to n samples: shared, never modify."""
    x = RR.clips(batch, L, 91)[b:b + 1]
    return x if n is None else x[:, :n].contiguous()


@functools.lru_cache(maxsize=8)
def reference(name, L, n=None, b=0, batch=1, rules=tuple(RULES)):
    """fp64 of both restatements on one clip, shared by the precisions: targets None and 0 of the rollouts, every rule set of the
    LRP at start_layer 0 and the default rules at start_layer 1."""
    x, mdl = clip(L, n, b, batch), ref_model(name)
    with torch.enable_grad():
        r = {"ar": AR.explain(x, mdl), "ar0": AR.explain(x, mdl, target=0)}
        r["lrp"] = {k: LR.explain(x, mdl, **RULES[k]) for k in rules}
        r["lrp_s1"] = LR.explain(x, mdl, start_layer=1)
    return r


def errors(got, ref):
    g, r = got.double().cpu().flatten(), ref.double().flatten()
    return ((g - r).abs().max() / (r.abs().max() + 1e-300)).item(), F.cosine_similarity(g, r, dim=0).item()


def close(got, ref, name, precision, what, worst):
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    if not bool(ref.any()):                                                      # an all-zero reference (a clamped map): zeros, exactly
        assert not bool(got.any()), what
        return
    err, cos = errors(got, ref)
    key = what.split(" [")[0]
    tol, cmin = PARENT_BAR.get((name, precision, key), TOL[precision])
    w = worst.setdefault(key, [0.0, 1.0])
    w[0], w[1] = max(w[0], err), min(w[1], cos)
    print(f"  {name} [{precision}] {what}: rel err {err:.2e} cosine {cos:.8f} (bars {tol:.0e} / {cmin})")
    assert torch.isfinite(got).all(), what
    assert err < tol and cos > cmin, (name, precision, what, err, cos)


def check_all(att, name, precision, x, r, worst, crop=None):
    """Every quantity of the four methods on the device clips ``x`` against the reference ``r``; ``crop=(kw, Tv)``: a ragged call,
    judged on the top-left Tv block, exact zeros elsewhere."""
    kw, Tv = ({}, None) if crop is None else crop
    ar, nl, B = r["ar"], att.eg.emb.nl, x.shape[0]

    def cut(t, dims):
        if Tv is None:
            return t
        idx = [slice(None)] * t.dim()
        for d in dims:
            rest = list(idx)
            rest[d] = slice(Tv, None)
            assert bool((t[tuple(rest)] == 0).all()), "not exactly zero past the clip's frames"
            idx[d] = slice(0, Tv)
        return t[tuple(idx)]
    sq = (-2, -1)
    for l in (0, nl - 1):                                                        # per-head maps at the first and last layer
        close(cut(att.attention_maps(x, l, **kw), sq), ar["A"][l], name, precision, f"A [layer {l}]", worst)
        close(cut(att.attention_maps(x, l, grad=True, **kw), sq), ar["GA"][l], name, precision, f"GA [layer {l}]", worst)
    for f in AR.FUSIONS:                                                         # the three fusions, maps and rollout
        close(cut(att.attention_maps(x, 0, f, **kw), sq), AR.fuse_heads(ar["A"][0], f), name, precision, f"A fused [{f}]", worst)
        rel, R = att.attention_rollout(x, f, return_joint=True, **kw)
        close(cut(R, sq), ar["R"][f], name, precision, f"R [{f}]", worst)
        close(cut(rel, (-1,)), ar["rel"][f], name, precision, f"rollout rel [{f}]", worst)
    rel, D = att.attention_grad_rollout(x, return_joint=True, **kw)
    close(cut(D, sq), ar["D"], name, precision, "D", worst)
    close(cut(rel, (-1,)), ar["rel_grad"], name, precision, "grad rollout rel", worst)
    for l in range(nl):                                                          # every layer's Abar on its own
        close(cut(att.attention_maps(x, l, "mean", grad=True, **kw), sq), ar["Abar"][l], name, precision, f"Abar [layer {l}]", worst)
    # start_layer > 0 (the references follow from the kept per-layer maps)
    rel1, R1 = att.attention_rollout(x, "mean", start_layer=1, return_joint=True, **kw)
    close(cut(R1, sq), AR.rollout(ar["A"], "mean", 1), name, precision, "R [start_layer 1]", worst)
    rel1, D1 = att.attention_grad_rollout(x, start_layer=1, return_joint=True, **kw)
    close(cut(D1, sq), AR.grad_rollout(ar["Abar"], 1), name, precision, "D [start_layer 1]", worst)
    # the four kinds of target: None above; 0 against its own reference; "predicted" and a tensor pick one of the two, bit for bit
    rel0, D0 = att.attention_grad_rollout(x, target=0, return_joint=True, **kw)
    close(cut(D0, sq), r["ar0"]["D"], name, precision, "D [target 0]", worst)
    assert B == 1
    pred_is_pos = bool(att.eg.forward(x, **kw)[0].view(-1)[0] > 0)               # the sign the engine itself predicts
    if abs(ar["logits"][0].item()) > 2e-2:                                       # beyond the f16 logit bar: the reference's sign too
        assert pred_is_pos == bool(ar["logits"][0] > 0)
    relp, Dp = att.attention_grad_rollout(x, target="predicted", return_joint=True, **kw)
    assert torch.equal(Dp, D if pred_is_pos else D0)
    relt, Dt = att.attention_grad_rollout(x, target=torch.zeros(B, dtype=torch.long), return_joint=True, **kw)
    assert torch.equal(Dt, D0) and torch.equal(relt, rel0)
    # LRP: default rules, each rule alone, all three with the identity rule, start_layer > 0, the targets
    for k, ref in r["lrp"].items():
        rel, R = att.transformer_lrp(x, return_hidden=True, **RULES[k], **kw)
        close(cut(R, (1,)), ref["R"], name, precision, f"lrp R [{k}]", worst)
        close(cut(rel, (1,)), ref["rel"], name, precision, f"lrp rel [{k}]", worst)
    rel, R = att.transformer_lrp(x, start_layer=1, return_hidden=True, **kw)
    close(cut(R, (1,)), r["lrp_s1"]["R"], name, precision, "lrp R [start_layer 1]", worst)
    rel = att.transformer_lrp(x, **kw)
    rel_0 = att.transformer_lrp(x, target=0, **kw)
    close(cut(rel_0, (1,)), -r["lrp"]["default"]["rel"], name, precision, "lrp rel [target 0]", worst)
    assert torch.equal(att.transformer_lrp(x, target="predicted", **kw), rel if pred_is_pos else rel_0)
    assert torch.equal(att.transformer_lrp(x, target=torch.ones(B, dtype=torch.long), **kw), rel)


def summary(tag, worst):
    print(f"{tag}: worst rel err / cosine: " + ", ".join(f"{k} {v[0]:.2e}/{v[1]:.6f}" for k, v in worst.items()))


@pytest.mark.parametrize("name,precision,L", CASES)
def test_long_maps_vs_fp64(gpu_device, name, precision, L):
    att = engine(name, precision)
    x = clip(L).to(gpu_device)
    worst = {}
    check_all(att, name, precision, x, reference(name, L), worst)
    summary(f"{name} [{precision}] L={L}", worst)
    # all rules off: layer_gradient_x_activation summed over the channels, bit for bit
    rel, R = att.transformer_lrp(x, ln_rule=False, attention_rule=False, return_hidden=True)
    gxa = att.layer_gradient_x_activation(x, 0)
    assert torch.equal(R, gxa)
    B, T, H = gxa.shape
    sums = torch.empty(B * T, dtype=torch.float32, device=gpu_device)
    att.eg.layer_tap(gxa.view(B * T, H), 1.0, want_out=False, row_sum=sums)
    assert torch.equal(rel, sums.view(B, T))
    # the input gradient is the same bits with and without attention_maps=
    eg, nl = att.eg, att.eg.emb.nl
    eg.forward(x)
    g = eg.backward(att.loss_scale)
    maps = torch.full((nl, B, T, T), NAN, device=gpu_device)
    assert torch.equal(eg.backward(att.loss_scale, attention_maps=(maps, 1)), g)
    assert bool(torch.isfinite(maps).all())


@pytest.mark.parametrize("name,precision", [(n, p) for n in LENGTHS for p in ("f32", "f16")])
def test_256_frames_are_the_default_chain(gpu_device, name, precision):
    """L = 82 319: all four methods with long_maps=True return the bits of a default HipAttribution, and both are held against
    fp64 with the bars above (the figures PARENT_BAR doubles where the default chain itself is over a bar)."""
    att, default = engine(name, precision), HipAttribution(LC.embedder(name, precision))
    x = clip(ANCHOR).to(gpu_device)
    for a in (att, default):
        assert a.eg.emb._lengths(ANCHOR)[-1] == 256
    pairs = [(lambda a: a.attention_maps(x, 0), "attention_maps"), (lambda a: a.attention_rollout(x, return_joint=True)[1], "rollout"),
             (lambda a: a.transformer_lrp(x, return_hidden=True)[1], "lrp")]
    if not (name == "head120" and precision == "f16"):                           # the fp16 whole-clip backward holds wide heads to 208 frames
        pairs += [(lambda a: a.attention_maps(x, 0, "max", grad=True), "grad maps"),
                  (lambda a: a.attention_grad_rollout(x, return_joint=True)[1], "grad rollout"),
                  (lambda a: a.transformer_lrp(x, attention_rule=False, return_hidden=True)[1], "lrp without the AH-rule")]
    for fn, what in pairs:
        assert torch.equal(fn(att), fn(default)), what
    if name == "head120" and precision == "f16":
        return
    worst = {}
    check_all(default, name, precision, x, reference(name, ANCHOR), worst)
    summary(f"default chain {name} [{precision}] L={ANCHOR}", worst)


def garbage(wave, lengths, value):
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = value
    return w


@pytest.mark.parametrize("name,precision", LC.TINY)
def test_ragged_batch_is_each_clip_alone(gpu_device, name, precision):
    """513, 299, 124 and 1 frames with lengths= on all four methods: each clip within the bars of fp64 on the cropped clip alone,
    exact zeros where defined, NaN / 1e30 in the padding changes no bit, each clip the bits of a B = 1 ragged call on that clip
    (at the batch's stride: below 257 frames of stride the chain's forward attention is the whole-clip ragged family, another
    arithmetic than the streamed one, as in tests/test_gpu_long_grad.py) and, above 256 frames, of the ragged and the non-ragged
    long call on the cropped clip at its own stride."""
    att, dev = engine(name, precision), gpu_device
    wave = RR.clips(len(RAGGED), max(RAGGED), 91)
    lens = list(RAGGED)
    frames = [RR.frames(att.eg.cfg, n) for n in lens]
    assert frames == [513, 299, 124, 1]
    kw = dict(lengths=lens)

    def run(w, kw_):
        out = {"A": att.attention_maps(w, 0, **kw_), "GA": att.attention_maps(w, 0, "mean", grad=True, **kw_)}
        out["rel"], out["R"] = att.attention_rollout(w, return_joint=True, **kw_)
        out["relg"], out["D"] = att.attention_grad_rollout(w, return_joint=True, **kw_)
        out["lrp"], out["lrpR"] = att.transformer_lrp(w, return_hidden=True, **kw_)
        return out
    got = run(wave.to(dev), kw)
    for value in (NAN, 1e30):
        other = run(garbage(wave, lens, value).to(dev), kw)
        for k in got:
            assert torch.equal(other[k], got[k]), (k, f"padding = {value} changed the result")
    square = {"A": (-2, -1), "GA": (-2, -1), "R": (-2, -1), "D": (-2, -1), "rel": (-1,), "relg": (-1,), "lrp": (1,), "lrpR": (1,)}
    worst = {}
    for b, (n, Tv) in enumerate(zip(lens, frames)):
        alone = run(wave[b:b + 1].to(dev), dict(lengths=[n]))
        x1 = wave[b:b + 1, :n].contiguous().to(dev)
        tight, plain = (run(x1, dict(lengths=[n])), run(x1, {})) if Tv > 256 else (None, None)
        for k, dims in square.items():
            t = got[k][b:b + 1]
            idx = [slice(None)] * t.dim()
            for d in dims:
                rest = list(idx)
                rest[d] = slice(Tv, None)
                assert bool((t[tuple(rest)] == 0).all()), (k, b, "not exactly zero past the clip's frames")
                idx[d] = slice(0, Tv)
            body = t[tuple(idx)]
            assert torch.equal(t, alone[k]), (k, b, "a clip depends on its batch")
            if plain is not None:
                assert torch.equal(body, tight[k]), (k, b, "stride 513 differs from the clip's own stride")
                assert torch.equal(body, plain[k]), (k, b, "the ragged call differs from the non-ragged long call")
        r = reference(name, max(RAGGED), n, b, len(RAGGED), rules=("default",))
        ar = r["ar"]
        sl = slice(b, b + 1)
        close(got["A"][sl, :, :Tv, :Tv], ar["A"][0], name, precision, f"A [clip {b}]", worst)
        close(got["GA"][sl, :Tv, :Tv], ar["Abar"][0], name, precision, f"Abar [clip {b}]", worst)
        close(got["R"][sl, :Tv, :Tv], ar["R"]["mean"], name, precision, f"R [clip {b}]", worst)
        close(got["rel"][sl, :Tv], ar["rel"]["mean"], name, precision, f"rollout rel [clip {b}]", worst)
        close(got["D"][sl, :Tv, :Tv], ar["D"], name, precision, f"D [clip {b}]", worst)
        close(got["relg"][sl, :Tv], ar["rel_grad"], name, precision, f"grad rollout rel [clip {b}]", worst)
        close(got["lrpR"][sl, :Tv], r["lrp"]["default"]["R"], name, precision, f"lrp R [clip {b}]", worst)
        close(got["lrp"][sl, :Tv], r["lrp"]["default"]["rel"], name, precision, f"lrp rel [clip {b}]", worst)
    summary(f"ragged {name} [{precision}]", worst)


@pytest.mark.parametrize("name", ["tiny_group", "tiny_layer"])
def test_conservation_on_a_bias_free_model(gpu_device, name):
    """All three rules on (GELU by identity), every bias, LayerNorm beta and the intercept zero: sum_t rel = +-F at 299 frames."""
    sd, cfg, coef, icpt = LR.zero_bias_model(ref_model(name))
    att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision="f32"), long_clips=True, long_maps=True)
    x = clip(96000).to(gpu_device)
    logit = att.eg.forward(x)[0].view(-1).cpu().double()
    for target, s0, sign in ((None, 0, 1.0), (0, 0, -1.0), (None, 1, 1.0)):
        rel = att.transformer_lrp(x, target=target, start_layer=s0, gelu_rule="identity").cpu().double()
        gap, mass = (rel.sum(-1) - sign * logit).abs(), rel.abs().sum(-1)
        print(f"{name} target={target} start_layer={s0}: |sum_t rel - (+-F)| {gap.tolist()} of sum_t |rel| {mass.tolist()}")
        assert bool((gap <= 1e-4 * mass).all())


def test_a_default_chain_still_refuses_with_nothing_allocated(gpu_device):
    att = HipAttribution(LC.embedder("tiny_group", "f32"), long_clips=True)
    x = clip(96000).to(gpu_device)
    att.input_gradient(x)                                                        # the long gradient chain itself works
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for call in (lambda: att.attention_maps(x, 0), lambda: att.attention_rollout(x), lambda: att.attention_grad_rollout(x),
                 lambda: att.transformer_lrp(x)):
        with pytest.raises(ValueError, match="attention maps need T <= 256 frames"):
            call()
    eg = att.eg
    pat = r"T x T attention kernels.*T <= 256 frames"
    with pytest.raises(_lib.AdvhError, match=pat):
        eg.attention_probs(0)
    with pytest.raises(_lib.AdvhError, match=pat):
        eg.backward(to_layer=0, attention_maps=(torch.zeros(1, device=gpu_device), 1))
    with pytest.raises(_lib.AdvhError, match=r"rules.*" + pat):
        eg.backward(to_layer=0, rules=LrpRules())
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                               # nothing was allocated by a refusal
    with pytest.raises(ValueError, match="lengths=.*long_maps=True"):
        att.attention_rollout(clip(16000).to(gpu_device), lengths=[8000])
    eg.forward(clip(16000).to(gpu_device), lengths=[8000])
    with pytest.raises(ValueError, match="ragged"):
        eg.attention_probs(0)
    with pytest.raises(ValueError, match="ragged"):
        eg.backward(to_layer=0, attention_maps=(torch.zeros(1, device=gpu_device), 1))
    with pytest.raises(ValueError, match="long_maps=True needs long_clips=True"):
        EmbedderGrad(LC.embedder("tiny_group", "f32"), long_maps=True)


CHILD = """
import sys, torch
sys.path[:0] = {paths!r}
import captum_saliency as cs
from addvisor_hip import synthetic as syn
dev = torch.device("cuda:0")
model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(dev)
x = syn.make_clips(1, 96000, seed=45).to(dev)
out = cs.explain_waves(model, x, method="transformer_lrp")
assert len(out) == 3 and all(p.shape == (1, 1) and bool(torch.isfinite(p).all()) for p in out)
assert model.hip_attribution().eg.long_maps is True
print("child ok", [p.item() for p in out])
"""


def test_explain_waves_on_six_seconds_in_a_fresh_process(gpu_device):
    """ADDVISOR_LONG_CLIPS=1 ADDVISOR_LONG_MAPS=1: explain_waves(method="transformer_lrp") takes a 6 s clip; with the first
    variable alone the same call raises the 256-frame ValueError."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "xai-audio-deepfakes_amd")]
    env = dict(os.environ, ADDVISOR_EMBEDDER="tiny", ADDVISOR_LONG_CLIPS="1", ADDVISOR_LONG_MAPS="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:], r.stderr[-2000:])
    assert r.returncode == 0 and "child ok" in r.stdout
    env.pop("ADDVISOR_LONG_MAPS")
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stderr[-600:])
    assert r.returncode != 0 and "attention maps need T <= 256 frames" in r.stderr and "child ok" not in r.stdout
