"""End to end: the gradient chain on clips longer than 256 frames (82 319 samples, 5.1 s), ``EmbedderGrad(long_clips=True)`` and
what is built on it.

Above 256 frames the chain's forward calls the streamed attention (csrc/attention_long.hip) and its backward the streamed
attention backward (csrc/attention_bwd_long.hip); every other launch is the one shorter clips take.  The four tiny models of
tests/test_gpu_long_clips.py -- group-norm / post-LN, layer-norm / pre-LN, head dim 64 and head dim 120 -- in both precisions, two
clips, at
    L =  82 320   T = 257, the first clip the default chain refuses,
    L =  96 000   T = 299, 6 s,
    L = 164 240   T = 513 (tiny_layer and head64): five blocks of 128 in every streaming loop, the last of one row,
against float64 autograd of the oracle on each clip alone (tests/ragged_grad_ref.py), and L = 82 319 (T = 256) as the anchor: with
``long_clips=True`` bit-identical to the default chain, on the path this feature leaves alone.

Bars, per clip and that clip's own max|ref| (tests/test_gpu_ragged_grad.py): f32 1e-4 and cosine > 0.999999; f16 3e-2 and cosine
> 0.999.  Where the EXISTING chain at L = 82 319 itself measures above a bar for a (model, precision, check), that case's bar is
twice the measurement (``PARENT_BAR``); the anchor test prints those measurements.  Every figure is printed in front of its
assertion.

Measured on an MI355X, worst over the models, lengths and clips of this file:
  f32  backward() 2.45e-6, seed 2.37e-6, to_layer 0 / 1 1.73e-6 / 2.12e-6, from_layer = 0 1.76e-6, cosine 1.00000000; the ragged
       batch <= 2.4e-6; Saliency / InputXGradient / IG / LayerGradientXActivation on 6 s <= 2.4e-6;
  f16  7.5e-3, 6.4e-3, 5.0e-3 / 4.0e-3, 4.5e-3, cosine >= 0.999995; ragged <= 4.5e-3; the attributions <= 3.8e-3.
The existing chain at L = 82 319: f32 <= 2.2e-6, f16 <= 3.4e-3 -- inside the bars, so ``PARENT_BAR`` is empty.  (head120, f16) has no
anchor gradient: the fp16 whole-clip backward holds head dims above 64 for T <= 208 frames, unchanged, with and without long_clips.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import layer_attr_ref
import ragged_grad_ref as GR
import ragged_ref as RR
import test_gpu_long_clips as LC
from addvisor_hip import _lib
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules
from oracle import attribution_ref
from test_gpu_attribution_baselines import DELTA_TOL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}      # (max |err| / max|ref| per clip, cosine): tests/test_gpu_ragged_grad.py
# (model, precision, check) -> (error bar, cosine bar): twice what the existing chain measures at L = 82 319
PARENT_BAR = {}
ANCHOR = 82319
LENGTHS = {"tiny_group": (82320, 96000), "tiny_layer": (82320, 96000, 164240), "head64": (82320, 96000, 164240), "head120": (82320, 96000)}
CASES = [(n, p, L) for n in LENGTHS for p in ("f32", "f16") for L in LENGTHS[n]]
CHECKS = ("plain", "seed", "to_layer0", "to_layer1", "lower")
LOWER_LOSS_SCALE = 256.0                                   # tests/test_gpu_ragged_grad.py: a unit seed at hidden_states[0]
RAGGED = LC.RAGGED                                         # (164240, 96000, 40000, 400): 513, 299, 124 and 1 frames
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def chain(name, precision, long_clips=True):
    return EmbedderGrad(LC.embedder(name, precision), long_clips=long_clips)


@functools.lru_cache(maxsize=None)
def seed_of(B):
    return torch.rand(B, generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0


@functools.lru_cache(maxsize=None)
def layer_seed_of(name, B, T):
    return torch.randn(B, T, LC.model(name)[0].hidden_size, generator=torch.Generator().manual_seed(6))


@functools.lru_cache(maxsize=None)
def reference(name, lengths, check):
    """fp64 autograd of the oracle on clip b of RR.clips(B, max(lengths), 91) cropped to lengths[b], alone.  Shared: never modify."""
    wave, mdl, B = RR.clips(len(lengths), max(lengths), 91), LC.model(name), len(lengths)
    with torch.enable_grad():
        if check == "plain":
            return GR.input_gradient(wave, lengths, mdl)[0]
        if check == "seed":
            return GR.input_gradient(wave, lengths, mdl, seed_of(B))[0]
        if check.startswith("to_layer"):
            return GR.layer_gradient(wave, lengths, mdl, int(check[-1]))
        return GR.lower_vjp(wave, lengths, mdl, layer_seed_of(name, B, RR.frames(mdl[0], max(lengths))))


def run(eg, name, check, wave, lengths, dev, clip=None):
    """One pass + the backward of ``check`` on ``wave`` (CPU); ``clip=(b, B, T)``: the seeds of clip b of a batch of B at T frames."""
    kw = {} if lengths is None else dict(lengths=lengths)
    B = wave.shape[0]
    b0, Bs, Ts = (0, B, RR.frames(eg.cfg, wave.shape[1])) if clip is None else clip
    if check == "lower":
        eg.forward(wave.to(dev), to_layer=0, **kw)
        S = layer_seed_of(name, Bs, Ts)[b0:b0 + B, :RR.frames(eg.cfg, wave.shape[1])].contiguous()
        return eg.backward(LOWER_LOSS_SCALE, from_layer=0, layer_seed=S.to(dev))
    eg.forward(wave.to(dev), **kw)
    if check == "plain":
        return eg.backward()
    if check == "seed":
        return eg.backward(seed=seed_of(Bs)[b0:b0 + B].to(dev))
    return eg.backward(to_layer=int(check[-1]))


def errors(got, ref):
    g, r = got.double().cpu().flatten(), ref.double().flatten()
    return ((g - r).abs().max() / (r.abs().max() + 1e-300)).item(), F.cosine_similarity(g, r, dim=0).item()


def test_shapes_are_what_the_kernels_need():
    cfg = LC.model("tiny_group")[0]
    assert [RR.frames(cfg, n) for n in (ANCHOR, 82320, 96000, 164240)] == [256, 257, 299, 513]
    assert [RR.frames(cfg, n) for n in RAGGED] == [513, 299, 124, 1]
    assert [LC.CONFIGS[n]().head_dim for n in LENGTHS] == [32, 32, 64, 120]


@pytest.mark.parametrize("name,precision,L", CASES)
def test_long_gradient_vs_fp64(gpu_device, name, precision, L):
    """backward(), a seeded backward, to_layer = 0 and 1, and from_layer = 0 with a layer_seed, two clips."""
    eg = chain(name, precision)
    wave = RR.clips(2, L, 91)
    T = RR.frames(eg.cfg, L)
    rows = []
    _lib.lib().advh_split_overflow(1)
    for check in CHECKS:
        got = run(eg, name, check, wave, None, gpu_device).cpu()
        assert torch.isfinite(got).all(), check
        ref = reference(name, (L, L), check)
        assert got.shape == ((2, T, eg.cfg.hidden_size) if check.startswith("to_layer") else (2, L))
        for b in range(2):
            e, c = errors(got[b], ref[b])
            print(f"{name} [{precision}] L={L} ({T} frames) {check} clip {b}: err {e:.3e} cosine {c:.8f}")
            rows.append((check, b, e, c))
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    for check, b, e, c in rows:
        tol, cos = PARENT_BAR.get((name, precision, check), TOL[precision])
        assert e <= tol and c > cos, (name, precision, L, check, b, e, c)


@pytest.mark.parametrize("name,precision", LC.ALL)
def test_256_frames_are_the_default_chain(gpu_device, name, precision):
    """The anchor: at L = 82 319 (T = 256) a ``long_clips`` chain launches what the default chain launches -- same bits -- and the
    default chain still refuses one sample more.  Prints the existing chain's own errors (the source of ``PARENT_BAR``)."""
    wave = RR.clips(2, ANCHOR, 91)
    rows = []
    if (name, precision) == ("head120", "f16"):              # unchanged: the fp16 whole-clip backward holds wide heads for T <= 208 frames
        for long_clips in (False, True):
            chain(name, precision, long_clips).forward(wave.to(gpu_device))
            with pytest.raises(_lib.AdvhError, match=r"head dim 120 > 64 is held for T <= 208 frames only \(T = 256"):
                chain(name, precision, long_clips).backward()
        return
    for check in CHECKS:
        a = run(chain(name, precision, False), name, check, wave, None, gpu_device)
        b = run(chain(name, precision, True), name, check, wave, None, gpu_device)
        assert torch.equal(a, b), check
        ref = reference(name, (ANCHOR, ANCHOR), check)
        for clip in range(2):
            e, c = errors(a[clip], ref[clip])
            print(f"{name} [{precision}] L={ANCHOR} (256 frames, the existing chain) {check} clip {clip}: err {e:.3e} cosine {c:.8f}")
            rows.append((check, e, c))
    workspaces = len(chain(name, precision, False)._ws)
    with pytest.raises(_lib.AdvhError, match=r"T <= 256 frames \(82319 samples\).*T = 257 \(82320 samples\)"):
        chain(name, precision, False).forward(RR.clips(1, 82320, 91).to(gpu_device))
    assert len(chain(name, precision, False)._ws) == workspaces
    for check, e, c in rows:
        tol, cos = PARENT_BAR.get((name, precision, check), TOL[precision])
        assert e <= tol and c > cos, (name, precision, check, e, c)


def garbage(wave, lengths, value):
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = value
    return w


@pytest.mark.parametrize("name,precision", LC.TINY)
def test_ragged_long_batch_is_each_clip_alone(gpu_device, name, precision):
    """513, 299, 124 and 1 frames in one batch: fp64 autograd on each cropped clip alone; exact zeros behind each length; content
    past a length changes no bit; a clip with more than 256 frames is bit-identical to the long chain on the cropped clip alone."""
    eg = chain(name, precision)
    cfg = eg.cfg
    wave = RR.clips(len(RAGGED), max(RAGGED), 91)
    frames = [RR.frames(cfg, n) for n in RAGGED]
    B, T = len(RAGGED), max(frames)
    rows = []
    _lib.lib().advh_split_overflow(1)
    for check in ("plain", "seed", "to_layer1", "lower"):
        got = run(eg, name, check, wave, RAGGED, gpu_device)
        for value in (NAN, 1e30):
            again = run(eg, name, check, garbage(wave, RAGGED, value), torch.tensor(RAGGED), gpu_device)
            assert torch.equal(again, got), (check, value, "content past the length changed the result")
        ref = reference(name, RAGGED, check)
        layer = check.startswith("to_layer")
        for b, n in enumerate(RAGGED):
            valid = frames[b] if layer else n
            assert bool((got[b, valid:] == 0).all()), (check, b, "values past the clip's length are not exactly zero")
            e, c = errors(got[b, :valid], ref[b] if layer else ref[b, :n])
            print(f"{name} [{precision}] ragged {check} clip {b} ({n} samples, {frames[b]} frames): err {e:.3e} cosine {c:.8f}")
            rows.append((check, b, e, c))
            if frames[b] > HipEmbedder.WHOLE_CLIP_MAX_FRAMES:
                one = run(eg, name, check, wave[b:b + 1, :n].contiguous(), None, gpu_device, clip=(b, B, T))
                assert torch.equal(one[0], got[b, :valid]), (check, b, "differs from the long chain on the cropped clip alone")
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    for check, b, e, c in rows:
        tol, cos = PARENT_BAR.get((name, precision, check), TOL[precision])
        assert e <= tol and c > cos, (name, precision, check, b, e, c)


@pytest.mark.parametrize("name,precision", LC.TINY)
def test_layer_chain_above_256_frames(gpu_device, name, precision):
    """forward_from, a neuron seed with row_scale and the refusals of the T x T kernels, at 299 frames."""
    eg = chain(name, precision)
    dev, L = gpu_device, 96000
    wave = RR.clips(2, L, 91).to(dev)
    T, H = RR.frames(eg.cfg, L), eg.cfg.hidden_size
    logits, _ = eg.forward(wave)
    g1 = eg.backward(to_layer=1)
    hid = eg.hidden(1)
    again, _ = eg.forward_from(1, hid)                       # layers 1 .. nl-1 on the same rows: the same launches on the same values
    assert torch.equal(again, logits)
    assert torch.equal(eg.backward(to_layer=1), g1)
    box = (3, T, 7, 0, H, 5)
    scale = torch.tensor([0.5, -2.0], device=dev)
    eg.forward(wave, to_layer=1)
    by_box = eg.backward(LOWER_LOSS_SCALE, from_layer=1, neuron=box, row_scale=scale)
    S = torch.zeros(2, T, H, device=dev)
    for b in range(2):
        S[b, box[0]:box[1]:box[2], box[3]:box[4]:box[5]] = scale[b]
    by_seed = eg.backward(LOWER_LOSS_SCALE, from_layer=1, layer_seed=S)      # powers of two: the same seed values
    assert torch.equal(by_box, by_seed) and torch.isfinite(by_box).all() and bool(by_box.any())
    eg.forward(wave)
    before = torch.cuda.memory_allocated()
    pat = r"T x T attention kernels.*T <= 256 frames"
    with pytest.raises(_lib.AdvhError, match=pat):
        eg.attention_probs(0)
    with pytest.raises(_lib.AdvhError, match=pat):
        eg.backward(to_layer=0, attention_maps=(torch.empty(0), 1))
    with pytest.raises(_lib.AdvhError, match=pat):
        eg.backward(to_layer=0, rules=LrpRules())
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize("name,precision", LC.TINY)
def test_attributions_on_six_seconds(gpu_device, name, precision):
    """HipAttribution(long_clips=True) at 96 000 samples against the restatements of oracle/attribution_ref.py and
    tests/layer_attr_ref.py at full length, and ``lengths=`` on a (96 000, 40 000) batch against each cropped clip."""
    cfg, sd, coef, icpt = LC.model(name)
    att = HipAttribution(LC.embedder(name, precision), long_clips=True)
    dev, L, N = gpu_device, 96000, 8
    wave = RR.clips(2, L, 91)
    w = wave.to(dev)
    with torch.enable_grad():
        refs = {"saliency": attribution_ref.saliency(wave, sd, cfg, coef, icpt),
                "ixg": attribution_ref.input_x_gradient(wave, sd, cfg, coef, icpt),
                "ig": attribution_ref.integrated_gradients(wave, sd, cfg, coef, icpt, n_steps=N),
                "lgxa": layer_attr_ref.layer_gradient_x_activation(wave, 1, (sd, cfg, coef, icpt))}
    ig, delta = att.integrated_gradients(w, n_steps=N, internal_batch_size=3, return_convergence_delta=True)
    got = {"saliency": att.saliency(w), "ixg": att.input_x_gradient(w), "ig": ig, "lgxa": att.layer_gradient_x_activation(w, 1)}
    rows = []
    for method, ref in refs.items():
        assert got[method].shape == ref.shape
        for b in range(2):
            e, c = errors(got[method][b], ref[b])
            print(f"{name} [{precision}] {method} on 6 s clip {b}: err {e:.3e} cosine {c:.8f}")
            rows.append((method, e, c))
    fx, f0 = layer_attr_ref.logit(wave, (sd, cfg, coef, icpt)).double(), layer_attr_ref.logit(torch.zeros_like(wave), (sd, cfg, coef, icpt)).double()
    want = refs["ig"].double().sum(1) - (fx - f0)
    rel, ab = DELTA_TOL[precision]
    print(f"{name} [{precision}] IG delta {delta.tolist()} | restatement {want.tolist()}")
    lengths = [96000, 40000]
    sal = att.saliency(garbage(wave, lengths, 1e30).to(dev), lengths=lengths)
    with torch.enable_grad():
        short = attribution_ref.saliency(wave[1:2, :40000].contiguous(), sd, cfg, coef, icpt)[0]
    assert torch.equal(sal[0], got["saliency"][0]) and bool((sal[1, 40000:] == 0).all())
    e, c = errors(sal[1, :40000], short)
    print(f"{name} [{precision}] saliency(lengths=(96000, 40000)) clip 1: err {e:.3e} cosine {c:.8f}")
    rows.append(("saliency lengths", e, c))
    for method, e, c in rows:
        assert e <= TOL[precision][0] and c > TOL[precision][1], (name, precision, method, e, c)
    assert ((delta.double().cpu() - want).abs() <= rel * (fx - f0).abs() + ab).all()
