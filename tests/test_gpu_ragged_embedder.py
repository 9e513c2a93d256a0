"""End to end: ``HipEmbedder.forward(wave, lengths=...)`` and the public wrappers on ragged batches.

One definition (tests/ragged_ref.py): the result for clip b is the oracle's for ``wave[b, :lengths[b]]`` run alone, unpadded.
The batch is the length table of tests/ragged_ref.py at L = 4000 (T = 12, 12, 7, 3, 2, 1, 1 frames) on ``tiny_config(stable=True)``
and ``tiny_config(stable=False)`` in both precisions, plus one wav2vec2-base case and one XLS-R-width case.

Bars: valid frames and logits within TOL_HID / TOL_LOGIT of tests/test_gpu_split.py (f32) and TOL_HID_MAX / TOL_LOGIT of
tests/test_gpu_embedder.py (f16), per clip, the figures printed in front of every assertion.  One length has a bar of its own:
the EXISTING forward, run alone on the cropped 400-sample clip of the group-norm tiny model in fp16 (one frame: the logit is one
row's dot product, nothing averages its fp16 error), is 1.160e-2 off the oracle's logit, above TOL_LOGIT = 1e-2 (measured on an
MI355X through ``forward(wave)``, the path this feature leaves alone).  Its bar is twice that measurement.  Every other
(model, precision, length) of this file is inside its bar on that path: f32 hidden <= 1.3e-5, logit <= 1.2e-5; f16 hidden
<= 1.8e-2, logit <= 9.7e-3.  The ragged call measured bit-identical to the existing forward on each cropped clip alone, for
every case of this file, so its errors against the oracle are those figures.
"""
import functools
import os

import pytest
import torch

import ragged_ref as RR
from addvisor_hip import _lib, runtime, synthetic as syn
from addvisor_hip.embedder import HipEmbedder
from oracle import wav2vec2_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 1e-4), "f16": (3e-2, 1e-2)}          # (hidden max |err|, logit / prob |err|): test_gpu_split.py | test_gpu_embedder.py
NAN = float("nan")
# (model, precision, samples) -> logit bar: twice what the existing forward measures on that clip alone (1.160e-2)
PARENT_LOGIT_BAR = {("tiny_group", "f16", 400): 2 * 1.160e-2}
CONFIGS = {
    "tiny_layer": lambda: syn.tiny_config(True),
    "tiny_group": lambda: syn.tiny_config(False),
    "base": lambda: syn.base_config(),
    "xlsr": lambda: syn.xlsr2b_config(num_hidden_layers=2, layer_index=2),
}
BATCHES = {"tiny_layer": (RR.L, RR.LENGTHS), "tiny_group": (RR.L, RR.LENGTHS), "base": (16000, (16000, 12345, 8000, 400)),
           "xlsr": (16000, (16000, 9000))}
TINY = [(n, p) for n in ("tiny_layer", "tiny_group") for p in ("f32", "f16")]
ALL = TINY + [("base", "f32"), ("base", "f16"), ("xlsr", "f32"), ("xlsr", "f16")]


@functools.lru_cache(maxsize=None)
def model(name):
    cfg = CONFIGS[name]()
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    return cfg, syn.embedder_weights(cfg), coef, icpt


@functools.lru_cache(maxsize=None)
def embedder(name, precision):
    cfg, sd, coef, icpt = model(name)
    return HipEmbedder(cfg, sd, coef, icpt, torch.device("cuda:0"), precision=precision)


@functools.lru_cache(maxsize=None)
def batch(name):
    L, lengths = BATCHES[name]
    return RR.clips(len(lengths), L, 91), lengths


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(hidden per clip, logits [B, 1], probs [B, 1]) of every clip run alone.  Shared: never modify."""
    cfg, sd, coef, icpt = model(name)
    wave, lengths = batch(name)
    hid = RR.per_clip_hidden(wave, lengths, sd, cfg)
    return (hid,) + tuple(RR.per_clip_classify(hid, coef, icpt))


def garbage(wave, lengths, value):
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = value
    return w


def check_against(tag, precision, hid, logit, prob, ref, lengths, frames):
    """Per clip: valid frames and the head against the reference, rows past the clip's frames exactly zero."""
    ref_h, ref_l, ref_p = ref
    tol_h, tol_l = TOL[precision]
    hid, logit, prob = hid.cpu(), logit.cpu(), prob.cpu()
    assert torch.isfinite(hid).all() and torch.isfinite(logit).all() and torch.isfinite(prob).all()
    rows = []
    for b, (n, Tb) in enumerate(zip(lengths, frames)):
        assert ref_h[b].shape[0] == Tb
        eh = (hid[b, :Tb] - ref_h[b]).abs().max().item()
        el = abs(logit[b, 0].item() - ref_l[b, 0].item())
        ep = abs(prob[b, 0].item() - ref_p[b, 0].item())
        rows.append((n, Tb, eh, el, ep))
        print(f"{tag} [{precision}] clip {b}: {n} samples, {Tb} frames: hidden max err {eh:.3e} | logit err {el:.3e} | prob err {ep:.3e}")
    for b, (n, Tb, eh, el, ep) in enumerate(rows):
        assert bool((hid[b, Tb:] == 0).all()), (b, "rows past the clip's frames are not exactly zero")
        bar_l = PARENT_LOGIT_BAR.get((tag.split()[0], precision, n), tol_l)
        assert eh <= tol_h and el <= bar_l and ep <= tol_l, (tag, precision, n, Tb, eh, el, ep)


@pytest.mark.parametrize("name,precision", ALL)
def test_ragged_forward_is_each_clip_alone(gpu_device, name, precision):
    """Assertions 1, 2 and 4: the oracle per clip; zeros behind; NaN and 1e30 past the length are zeros past the length."""
    emb = embedder(name, precision)
    wave, lengths = batch(name)
    frames = emb.frame_lengths(lengths)
    _lib.lib().advh_split_overflow(1)
    out = emb.forward(wave.to(gpu_device), lengths=lengths)
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    check_against(name, precision, *out, oracle(name), lengths, frames)
    for value in (NAN, 1e30, 0.0):
        again = emb.forward(garbage(wave, lengths, value).to(gpu_device), lengths=torch.tensor(lengths))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(again, out)), (value, "content past the length changed the result")
    assert _lib.lib().advh_split_overflow(0) == 0


@pytest.mark.parametrize("name,precision", ALL)
def test_full_lengths_are_the_padded_forward(gpu_device, name, precision):
    """Assertion 3: lengths = [L] * B is bit-identical to forward(wave)."""
    emb = embedder(name, precision)
    wave, lengths = batch(name)
    w = wave.to(gpu_device)
    plain = emb.forward(w)
    full = emb.forward(w, lengths=[wave.shape[1]] * wave.shape[0])
    assert all(torch.equal(a, b) for a, b in zip(full, plain))
    assert emb.forward(w, lengths=[wave.shape[1]] * wave.shape[0], want_hidden=False)[0] is None


@pytest.mark.parametrize("name,precision", TINY)
def test_clip_zero_does_not_see_its_neighbours(gpu_device, name, precision):
    """Assertion 5: clip 0 is bit-identical when the other clips' lengths and contents change."""
    emb = embedder(name, precision)
    wave, lengths = batch(name)
    a = emb.forward(wave.to(gpu_device), lengths=lengths)
    other = wave.clone()
    other[1:] = RR.clips(len(lengths), wave.shape[1], 17)[1:] * 3.0
    swapped = (lengths[0],) + tuple(reversed(lengths[1:]))
    b = emb.forward(other.to(gpu_device), lengths=swapped)
    c = emb.forward(other[:2].contiguous().to(gpu_device), lengths=[lengths[0], 400])            # another batch size
    for o in (b, c):
        assert all(torch.equal(x[0], y[0]) for x, y in zip(o, a))
    # and a short clip in slot 0 likewise
    short = emb.forward(wave.flip(0).contiguous().to(gpu_device), lengths=tuple(reversed(lengths)))
    alone = emb.forward(wave[-1:].contiguous().to(gpu_device), lengths=lengths[-1:])
    assert all(torch.equal(x[0], y[0]) for x, y in zip(short, alone))


@pytest.mark.parametrize("name,precision", TINY)
def test_against_the_existing_forward_on_each_cropped_clip(gpu_device, name, precision):
    """Assertion 6: the padded-path forward on ``wave[b, :lengths[b]]`` alone (B = 1), within the same tolerance."""
    emb = embedder(name, precision)
    wave, lengths = batch(name)
    frames = emb.frame_lengths(lengths)
    hid, logit, prob = (t.cpu() for t in emb.forward(wave.to(gpu_device), lengths=lengths))
    alone = [tuple(t.cpu() for t in emb.forward(wave[b:b + 1, :n].contiguous().to(gpu_device))) for b, n in enumerate(lengths)]
    ref = ([a[0][0] for a in alone], torch.cat([a[1] for a in alone]), torch.cat([a[2] for a in alone]))
    check_against(name + " vs forward alone", precision, hid, logit, prob, ref, lengths, frames)


@pytest.mark.parametrize("name,precision", TINY)
def test_no_state_is_left_between_calls(gpu_device, name, precision):
    """Assertion 7: forward(wave) and HipAttribution.saliency(wave) give the same bits before and after a ragged call, and the
    feature-encoder buffers (their zero filler and slack rows included) are the same bits after forward(wave)."""
    from addvisor_hip.attribution import HipAttribution
    from addvisor_hip.embedder import FE_SLACK_ROWS
    emb = embedder(name, precision)
    att = HipAttribution(emb)
    wave, lengths = batch(name)
    w = wave.to(gpu_device)
    B, L = wave.shape
    before = emb.forward(w)
    ws = emb._ws[(B, L, 0)]
    fe_before = [t.clone() for t in ws["fe"]]
    sal_before = att.saliency(w).clone()
    rag = emb.forward(garbage(wave, lengths, 1e30).to(gpu_device), lengths=lengths)
    torch.cuda.synchronize()
    assert len(emb._ws) >= 1 and emb._ws[(B, L, 0)] is ws                    # the padded call's workspace and plans
    C = emb.cfg.conv_dim
    for i, t in enumerate(ws["fe"]):                                         # slack rows behind the buffers: still zero
        assert bool((t[..., B * ws["P"][i] * C[i]:] == 0).all()) and t.shape[-1] == B * ws["P"][i] * C[i] + FE_SLACK_ROWS * max(C)
    assert all(p > n for p, n in zip(ws["P"], ws["Ls"]))                     # every layer keeps a filler row per clip
    after = emb.forward(w)
    fe_after = [t.clone() for t in ws["fe"]]
    sal_after = att.saliency(w)
    assert all(torch.equal(x, y) for x, y in zip(after, before))
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(fe_after, fe_before))
    assert torch.equal(sal_after, sal_before)
    assert torch.isfinite(rag[1]).all()


def test_value_errors_fire_before_any_launch(gpu_device):
    """Assertion 8: a shape that was never planned stays unplanned."""
    emb = embedder("tiny_layer", "f32")
    w = torch.zeros(3, 4321, device=gpu_device)
    bad = [dict(lengths=[4321, 400]), dict(lengths=[4321, 400.0, 400]), dict(lengths=[4321, 4322, 400]), dict(lengths=[4321, 399, 400]),
           dict(lengths=[4321, 400, 400], length=4321), dict(lengths=torch.tensor([4321.0, 400.0, 400.0])), dict(lengths=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            emb.forward(w, **kw)
    with pytest.raises(ValueError, match=r"clip 1 has 399 samples.*shortest supported length is 400"):
        emb.forward(w, lengths=[4321, 399, 400])
    assert not any(k[:2] == (3, 4321) for k in emb._ws)


@pytest.fixture
def tiny_layer_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny_layer"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_public_wrappers(gpu_device, tiny_layer_runtime):
    """Assertion 9: classify(lengths=), Wav2vec2LogReg.forward(lengths=), wav2vec2(attention_mask=) and pad_clips."""
    import audioprocessor
    import captum_saliency as cs
    emb = runtime.hip_embedder()
    precision = emb.precision
    wave, lengths = batch("tiny_layer")
    frames = emb.frame_lengths(lengths)
    w = garbage(wave, lengths, 1e30).to(gpu_device)
    hid, logit, prob = emb.forward(w, lengths=lengths)
    ap = audioprocessor.AudioProcessor(audio_length=1)
    feats = ap.extract_features(w, lengths=lengths)
    l2, p2 = ap.classify(w, lengths=lengths)
    assert torch.equal(feats, hid) and torch.equal(l2, logit) and torch.equal(p2, prob)
    model_ = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    assert torch.equal(model_(w, lengths=lengths), logit) and torch.equal(model_.forward(w[:1, :lengths[0]]), logit[:1])
    padded, plen = audioprocessor.pad_clips([wave[b, :n] for b, n in enumerate(lengths)])
    assert plen == list(lengths) and torch.equal(padded, garbage(wave, lengths, 0.0))
    l3, p3 = ap.classify(padded, lengths=plen)
    assert torch.equal(l3, logit) and torch.equal(p3, prob)
    # the drop-in model call: input_values normalised over the valid part (as HF's feature extractor delivers them), 0 / 1 mask
    x = torch.zeros_like(wave)
    mask = torch.zeros(wave.shape, dtype=torch.long)
    for b, n in enumerate(lengths):
        x[b, :n] = wav2vec2_ref.zero_mean_unit_var_norm(wave[b:b + 1, :n])[0]
        mask[b, :n] = 1
    hs = audioprocessor.wav2vec2(x.to(gpu_device), attention_mask=mask.to(gpu_device), output_hidden_states=True).hidden_states[emb.cfg.layer_index]
    ref_h, _, _ = oracle("tiny_layer")
    for b, Tb in enumerate(frames):
        e = (hs[b, :Tb].cpu() - ref_h[b]).abs().max().item()
        print(f"wav2vec2(attention_mask) clip {b}: hidden max err {e:.3e}")
        assert e <= TOL[precision][0] and bool((hs[b, Tb:] == 0).all())
    holes = mask.clone()
    holes[2, 3000] = 1
    with pytest.raises(ValueError, match="holes"):
        audioprocessor.wav2vec2(x.to(gpu_device), attention_mask=holes)
