"""End to end: ``EmbedderGrad.forward(wave, lengths=...)`` + ``backward(...)`` on ragged batches.

One definition (tests/ragged_grad_ref.py): what the chain returns for clip b is float64 autograd of the oracle on
``wave[b, :lengths[b]]`` run alone, zero-filled to ``L``.  Models and lengths: the tiny layer-norm (pre-LN), tiny group-norm
(post-LN) and depth-9 tiny models at L = 4000 with the seven lengths of ``ragged_ref.TABLE`` in one batch, both precisions; in
f32 also wav2vec2-base at (16000, 12345, 8000, 400) and the XLS-R width with two layers at (16000, 9000) (head dim 120: the
fp32-MFMA backward kernel).

Bars, per clip over ``dx[b, :lengths[b]]`` and that clip's own max|ref| (tests/test_gpu_backward.py): f32 1e-4 and cosine
> 0.999999; f16 3e-2 and cosine > 0.999.  Where the EXISTING chain on the cropped clip alone (B = 1) itself measures above a bar,
that case's bar is twice the measurement (``PARENT_BAR``).  Every ragged result is also asserted bit-identical to that same
B = 1 run of the existing chain, so its error against the reference is the existing chain's.

Measured on an MI355X (worst clip per model; the existing chain alone and the ragged chain gave the same bits in every case, so
``PARENT_BAR`` is empty -- the one-frame fp16 clips measure 3.5e-3 .. 3.7e-3, inside the bar):
  f32  backward() <= 4.4e-6, seed <= 4.8e-6, to_layer <= 1.5e-6, from_layer = 0 <= 1.7e-6 (tiny models, wav2vec2-base, XLS-R width),
       cosine 1.00000000;
  f16  backward() <= 5.3e-3, seed <= 5.4e-3, to_layer <= 2.7e-3, from_layer = 0 <= 3.7e-3, cosine >= 0.999991.
The table per model is in DESIGN 4.32.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import ragged_grad_ref as GR
import ragged_ref as RR
from addvisor_hip import _lib
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}      # (max |err| / max|ref| per clip, cosine): tests/test_gpu_backward.py
# (model, precision, check, samples) -> (error bar, cosine bar): twice what the existing chain measures on that clip alone
PARENT_BAR = {}
BATCHES = {"tiny_layer": (RR.L, RR.LENGTHS), "tiny_group": (RR.L, RR.LENGTHS), "tiny_layer_depth9": (RR.L, RR.LENGTHS),
           "base": (16000, (16000, 12345, 8000, 400)), "xlsr": (16000, (16000, 9000))}
TINY = [(n, p) for n in ("tiny_layer", "tiny_group", "tiny_layer_depth9") for p in ("f32", "f16")]
ALL = TINY + [("base", "f32"), ("xlsr", "f32")]
TO_LAYER = 1
# a unit seed at hidden_states[0] is far larger than the logit's coef / T: the scale tests/test_gpu_fe_backward.py uses for it (the
# default 4096 leaves the split format's range in the group-norm model's feature encoder and raises SplitRangeError, as it does unpadded)
LOWER_LOSS_SCALE = 256.0
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def chain(name, precision):
    cfg, sd, coef, icpt = GR.model(name)
    return EmbedderGrad(HipEmbedder(cfg, sd, coef, icpt, torch.device("cuda:0"), precision=precision))


@functools.lru_cache(maxsize=None)
def batch(name):
    L, lengths = BATCHES[name]
    return RR.clips(len(lengths), L, 91), lengths


@functools.lru_cache(maxsize=None)
def seed_of(name):
    B = len(BATCHES[name][1])
    return torch.rand(B, generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0


@functools.lru_cache(maxsize=None)
def layer_seed_of(name):
    cfg = GR.model(name)[0]
    L, lengths = BATCHES[name]
    return torch.randn(len(lengths), RR.frames(cfg, L), cfg.hidden_size, generator=torch.Generator().manual_seed(6))


@functools.lru_cache(maxsize=None)
def reference(name, check):
    """The fp64 reference of one check.  Shared: never modify."""
    wave, lengths = batch(name)
    mdl = GR.model(name)
    with torch.enable_grad():
        if check == "plain":
            return GR.input_gradient(wave, lengths, mdl)[0]
        if check == "seed":
            return GR.input_gradient(wave, lengths, mdl, seed_of(name))[0]
        if check == "to_layer":
            return GR.layer_gradient(wave, lengths, mdl, TO_LAYER)
        return GR.lower_vjp(wave, lengths, mdl, layer_seed_of(name))


def garbage(wave, lengths, value):
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = value
    return w


def run(eg, name, check, wave, lengths, dev):
    """One ragged pass + the backward of ``check`` on ``wave`` (CPU) with ``lengths`` (None: the padded call)."""
    kw = {} if lengths is None else dict(lengths=lengths)
    B = wave.shape[0]
    if check == "lower":
        eg.forward(wave.to(dev), to_layer=0, **kw)
        return eg.backward(LOWER_LOSS_SCALE, from_layer=0, layer_seed=layer_seed_of(name)[:B].to(dev))
    eg.forward(wave.to(dev), **kw)
    if check == "plain":
        return eg.backward()
    if check == "seed":
        return eg.backward(seed=seed_of(name)[:B].to(dev))
    return eg.backward(to_layer=TO_LAYER)


def alone(eg, name, check, wave, b, n, dev):
    """The EXISTING chain on clip b cropped to n samples, run alone (B = 1, no lengths)."""
    cfg = eg.cfg
    x = wave[b:b + 1, :n].contiguous().to(dev)
    if check == "lower":
        eg.forward(x, to_layer=0)
        return eg.backward(LOWER_LOSS_SCALE, from_layer=0, layer_seed=layer_seed_of(name)[b:b + 1, :RR.frames(cfg, n)].contiguous().to(dev))
    eg.forward(x)
    if check == "plain":
        return eg.backward()
    if check == "seed":
        return eg.backward(seed=seed_of(name)[b:b + 1].to(dev))
    return eg.backward(to_layer=TO_LAYER)


def errors(got, ref):
    g, r = got.double().flatten(), ref.double().flatten()
    return ((g - r).abs().max() / r.abs().max()).item(), F.cosine_similarity(g, r, dim=0).item()


@pytest.mark.parametrize("check", ["plain", "seed", "to_layer", "lower"])
@pytest.mark.parametrize("name,precision", ALL)
def test_ragged_gradient_is_each_clip_alone(gpu_device, name, precision, check):
    """Against the fp64 reference at the chain's bars, exact zeros behind, and the existing chain's bits on each cropped clip."""
    eg = chain(name, precision)
    wave, lengths = batch(name)
    cfg = eg.cfg
    frames = [RR.frames(cfg, n) for n in lengths]
    _lib.lib().advh_split_overflow(1)
    got = run(eg, name, check, wave, lengths, gpu_device).cpu()
    assert _lib.lib().advh_split_overflow(0) == 0
    assert torch.isfinite(got).all()
    ref = reference(name, check)
    layer = check == "to_layer"
    rows = []
    for b, n in enumerate(lengths):
        valid = frames[b] if layer else n
        one = alone(eg, name, check, wave, b, n, gpu_device).cpu()[0]
        r = ref[b] if layer else ref[b, :n]
        e, c = errors(got[b, :valid], r)
        e1, c1 = errors(one, r)
        same = torch.equal(got[b, :valid], one)
        print(f"{name} [{precision}] {check} clip {b} ({n} samples, {frames[b]} frames): err {e:.3e} cosine {c:.8f} | "
              f"existing chain alone: err {e1:.3e} cosine {c1:.8f} | bit-identical {same}")
        rows.append((b, n, valid, e, c, same))
    for b, n, valid, e, c, same in rows:
        assert bool((got[b, valid:] == 0).all()), (b, "values past the clip's length are not exactly zero")
        tol, cos = PARENT_BAR.get((name, precision, check, n), TOL[precision])
        assert e <= tol and c > cos, (name, precision, check, n, e, c)
        assert same, (name, precision, check, n, "differs from the existing chain on the cropped clip alone")


@pytest.mark.parametrize("name,precision", TINY)
def test_padding_content_and_call_order_change_no_bit(gpu_device, name, precision):
    """NaN / 1e30 past the lengths change no bit and leave the overflow flag clear; padded and ragged calls alternating on one
    EmbedderGrad equal fresh-instance results bit for bit; to_layer hidden states have zero tail rows."""
    eg = chain(name, precision)
    wave, lengths = batch(name)
    dev = gpu_device
    cfg, sd, coef, icpt = GR.model(name)
    fresh = lambda: EmbedderGrad(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))
    rag0 = {c: run(fresh(), name, c, wave, lengths, dev) for c in ("plain", "lower")}
    pad0 = {c: run(fresh(), name, c, wave, None, dev) for c in ("plain", "lower")}
    _lib.lib().advh_split_overflow(1)
    for value in (NAN, 1e30):
        for c in ("plain", "seed", "to_layer", "lower"):
            a = run(eg, name, c, wave, lengths, dev)
            b = run(eg, name, c, garbage(wave, lengths, value), torch.tensor(lengths), dev)
            assert torch.equal(a, b), (value, c, "content past the length changed the result")
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    for c in ("plain", "lower"):                             # ragged, padded, ragged, padded on ONE instance
        assert torch.equal(run(eg, name, c, garbage(wave, lengths, 1e30), lengths, dev), rag0[c])
        assert torch.equal(run(eg, name, c, wave, None, dev), pad0[c])
        assert torch.equal(run(eg, name, c, wave, lengths, dev), rag0[c])
        assert torch.equal(run(eg, name, c, wave, None, dev), pad0[c])
    hid = eg.forward(garbage(wave, lengths, NAN).to(dev), to_layer=TO_LAYER, lengths=lengths)
    for b, n in enumerate(lengths):
        Tb = RR.frames(cfg, n)
        assert bool((hid[b, Tb:] == 0).all()) and torch.isfinite(hid[b, :Tb]).all()
    assert torch.equal(eg.hidden(TO_LAYER), hid)


@pytest.mark.parametrize("name,precision", ALL)
def test_full_lengths_are_the_padded_call(gpu_device, name, precision):
    eg = chain(name, precision)
    wave, lengths = batch(name)
    full = [wave.shape[1]] * wave.shape[0]
    for c in ("plain", "seed", "to_layer", "lower"):
        assert torch.equal(run(eg, name, c, wave, full, gpu_device), run(eg, name, c, wave, None, gpu_device)), c
    w = wave.to(gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(eg.forward(w, lengths=full), eg.forward(w)))


def test_a_seed_or_box_past_the_frames_is_ignored(gpu_device):
    """``layer_seed`` rows and a neuron box reaching past ``T_b`` do not reach the gradient."""
    name = "tiny_layer"
    eg = chain(name, "f32")
    wave, lengths = batch(name)
    cfg = eg.cfg
    w = wave.to(gpu_device)
    S = layer_seed_of(name).clone()
    eg.forward(w, to_layer=0, lengths=lengths)
    a = eg.backward(LOWER_LOSS_SCALE, from_layer=0, layer_seed=S.to(gpu_device))
    for b, n in enumerate(lengths):
        S[b, RR.frames(cfg, n):] = 100.0
    b_ = eg.backward(LOWER_LOSS_SCALE, from_layer=0, layer_seed=S.to(gpu_device))
    assert torch.equal(a, b_)
    T, H = S.shape[1:]
    whole = eg.backward(16.0, from_layer=0, neuron=(0, T, 1, 0, H, 1))
    one = eg.backward(16.0, from_layer=0, neuron=(0, 1, 1, 0, H, 1))
    short = [b for b, n in enumerate(lengths) if RR.frames(cfg, n) == 1]
    assert short and all(torch.equal(whole[b], one[b]) for b in short)      # a one-frame clip: the box's other frames do not exist


def test_arguments_after_a_ragged_pass(gpu_device):
    from addvisor_hip.embedder_grad import LrpRules
    eg = chain("tiny_layer", "f32")
    wave, lengths = batch("tiny_layer")
    w = wave.to(gpu_device)
    B, T, H = w.shape[0], RR.frames(eg.cfg, RR.L), eg.cfg.hidden_size
    with pytest.raises(ValueError, match="not both"):
        eg.forward(w, length=RR.L, lengths=lengths)
    eg.forward(w, lengths=lengths)
    with pytest.raises(ValueError, match="attention_maps"):
        eg.backward(to_layer=0, attention_maps=(torch.empty(1, B, T, T, device=gpu_device), 1))
    with pytest.raises(ValueError, match="rules"):
        eg.backward(to_layer=0, rules=LrpRules())
    with pytest.raises(RuntimeError, match="ragged"):
        eg.forward_from(0, torch.zeros(B, T, H, device=gpu_device))
    eg.forward(w)                                            # a padded pass lifts the refusals
    eg.backward(to_layer=0, rules=LrpRules())
    eg.forward_from(0, torch.zeros(B, T, H, device=gpu_device))
