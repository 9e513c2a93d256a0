"""End to end: clips longer than 256 frames (82 319 samples, 5.1 s) through ``HipEmbedder.forward`` and what is built on it.

Above 256 frames the forward calls the streamed attention (csrc/attention_long.hip); every other launch is the one shorter clips
take, and none of them had run beyond 249 frames before.  Four tiny models -- group-norm / post-LN, layer-norm / pre-LN, and the
head-dim-64 and head-dim-120 variants -- in both precisions, two clips, at
    L =  82 320   T = 257, the first clip the whole-clip kernels refuse,
    L =  96 000   T = 299, 6 s,
    L = 164 240   T = 513, three key blocks of 256 and a fifth query block of one row,
against ``oracle/wav2vec2_ref`` on the CPU, and L = 82 319 (T = 256) as the anchor: bit-identical to two batch-1 calls, on the
path this feature leaves alone.

Bars, the project's stated ones: f32 hidden 1e-4 and logit 1e-4 (tests/test_gpu_split.py), f16 hidden 3e-2 and logit 1e-2
(tests/test_gpu_embedder.py); the pipeline's are those of tests/test_gpu_pipeline.py, the occlusion's that of
tests/test_gpu_ablation.py.  Every figure is printed in front of its assertion.

Measured on an MI355X, worst over the models, lengths and clips of this file: f32 hidden 1.05e-5, logit 3.9e-6; f16 hidden 2.0e-2,
logit 8.8e-3.  ExplainPipeline(audio_length=6): f32 probabilities 3.6e-7, mask 5.7e-6; f16 8.3e-4 / 5.3e-3.  Occlusion on 6 s:
f32 1.3e-6, f16 3.8e-3.
"""
import functools
import os

import pytest
import torch

import ablation_ref
import ragged_ref as RR
from addvisor_hip import _lib, pipeline as P, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from oracle import lmac_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 1e-4), "f16": (3e-2, 1e-2)}          # (hidden max |err|, logit / prob |err|)
TOL_PIPE = {"f32": dict(prob=1e-4, mask=2e-5), "f16": dict(prob=1e-2, mask=1.5e-2)}      # tests/test_gpu_pipeline.py
TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}                     # tests/test_gpu_ablation.py
NAN = float("nan")
CONFIGS = {
    "tiny_group": lambda: syn.tiny_config(False),
    "tiny_layer": lambda: syn.tiny_config(True),
    "head64": lambda: syn.tiny_config(False, hidden_size=128, num_attention_heads=2, intermediate_size=256),
    "head120": lambda: syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480),
}
LENGTHS = (82320, 96000, 164240)
FRAMES = {82319: 256, 82320: 257, 96000: 299, 164240: 513}
RAGGED = (164240, 96000, 40000, 400)
ALL = [(n, p) for n in CONFIGS for p in ("f32", "f16")]
TINY = [(n, p) for n in ("tiny_group", "tiny_layer") for p in ("f32", "f16")]


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
def oracle(name, lengths):
    """(hidden per clip, logits [B, 1], probs [B, 1]) of clip b of RR.clips(B, max(lengths), 91) cropped to lengths[b], run
    alone.  Shared between the precisions: never modify."""
    cfg, sd, coef, icpt = model(name)
    hid = RR.per_clip_hidden(RR.clips(len(lengths), max(lengths), 91), lengths, sd, cfg)
    return (hid,) + tuple(RR.per_clip_classify(hid, coef, icpt))


def check_against(tag, precision, out, ref, frames):
    ref_h, ref_l, ref_p = ref
    tol_h, tol_l = TOL[precision]
    hid, logit, prob = (t.cpu() for t in out)
    assert torch.isfinite(hid).all() and torch.isfinite(logit).all() and torch.isfinite(prob).all()
    rows = []
    for b, Tb in enumerate(frames):
        assert ref_h[b].shape[0] == Tb
        eh = (hid[b, :Tb] - ref_h[b]).abs().max().item()
        el = abs(logit[b, 0].item() - ref_l[b, 0].item())
        ep = abs(prob[b, 0].item() - ref_p[b, 0].item())
        rows.append((Tb, eh, el, ep))
        print(f"{tag} [{precision}] clip {b}: {Tb} frames: hidden max err {eh:.3e} | logit err {el:.3e} | prob err {ep:.3e}")
    for b, (Tb, eh, el, ep) in enumerate(rows):
        assert bool((hid[b, Tb:] == 0).all()), (b, "rows past the clip's frames are not exactly zero")
        assert eh <= tol_h and el <= tol_l and ep <= tol_l, (tag, precision, b, Tb, eh, el, ep)


def test_frame_counts():
    cfg = model("tiny_group")[0]
    assert {n: RR.frames(cfg, n) for n in FRAMES} == FRAMES
    assert all(CONFIGS[n]().conv_kernel == cfg.conv_kernel and CONFIGS[n]().conv_stride == cfg.conv_stride for n in CONFIGS)
    assert [CONFIGS[n]().head_dim for n in CONFIGS] == [32, 32, 64, 120]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name,precision", ALL)
def test_long_forward_vs_oracle(gpu_device, name, precision, L):
    emb = embedder(name, precision)
    wave = RR.clips(2, L, 91)
    _lib.lib().advh_split_overflow(1)
    out = emb.forward(wave.to(gpu_device))
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    assert out[0].shape == (2, FRAMES[L], emb.cfg.hidden_size)
    check_against(f"{name} L={L}", precision, out, oracle(name, (L, L)), (FRAMES[L],) * 2)


@pytest.mark.parametrize("name,precision", ALL)
def test_256_frames_stay_on_the_whole_clip_path(gpu_device, name, precision):
    """The regression anchor: the longest clip the whole-clip kernels take, as a batch of two and as two batch-1 calls."""
    emb = embedder(name, precision)
    wave = RR.clips(2, 82319, 91).to(gpu_device)
    both = emb.forward(wave)
    assert both[0].shape[1] == 256
    for b in range(2):
        one = emb.forward(wave[b:b + 1].contiguous())
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip(both, one)), b
    check_against(f"{name} L=82319", precision, both, oracle(name, (82319, 82319)), (256, 256))


def garbage(wave, lengths, value):
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = value
    return w


@pytest.mark.parametrize("name,precision", TINY)
def test_ragged_long_batch_is_each_clip_alone(gpu_device, name, precision):
    """513, 299, 124 and 1 frames in one batch: the oracle on each cropped clip alone; padded rows exactly zero; content past a
    length changes no bit; a clip with more than 256 frames is bit-identical to ``forward`` on the cropped clip alone."""
    emb = embedder(name, precision)
    wave = RR.clips(len(RAGGED), max(RAGGED), 91)
    frames = emb.frame_lengths(RAGGED)
    assert frames == [513, 299, 124, 1]
    _lib.lib().advh_split_overflow(1)
    out = emb.forward(wave.to(gpu_device), lengths=RAGGED)
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(0) == 0
    check_against(f"{name} ragged", precision, out, oracle(name, RAGGED), frames)
    for value in (NAN, 1e30):
        again = emb.forward(garbage(wave, RAGGED, value).to(gpu_device), lengths=torch.tensor(RAGGED))
        assert all(torch.equal(a, b) for a, b in zip(again, out)), (value, "content past the length changed the result")
    for b, (n, Tb) in enumerate(zip(RAGGED, frames)):
        if Tb > HipEmbedder.WHOLE_CLIP_MAX_FRAMES:
            hid, logit, prob = emb.forward(wave[b:b + 1, :n].contiguous().to(gpu_device))
            assert torch.equal(hid[0], out[0][b, :Tb]) and torch.equal(logit[0], out[1][b]) and torch.equal(prob[0], out[2][b]), b


@pytest.fixture
def tiny_layer_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny_layer"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_audioprocessor_takes_six_seconds(gpu_device, tiny_layer_runtime):
    import audioprocessor
    emb = runtime.hip_embedder()
    wave = RR.clips(2, 96000, 91)
    ap = audioprocessor.AudioProcessor(audio_length=6)
    feats = ap.extract_features(wave.to(gpu_device))
    logits, probs = ap.classify(wave.to(gpu_device))
    assert feats.shape == (2, 299, emb.cfg.hidden_size)
    check_against("AudioProcessor(audio_length=6)", emb.precision, (feats, logits, probs), oracle("tiny_layer", (96000, 96000)), (299, 299))
    l2, p2 = ap.classify(wave.to(gpu_device), lengths=[96000, 90000])
    assert torch.equal(l2[0], logits[0]) and torch.isfinite(l2).all() and torch.isfinite(p2).all()


@functools.lru_cache(maxsize=None)
def explain_setup():
    cfg, emb_sd, coef, icpt = model("tiny_group")
    unet_sd = syn.unet_weights()
    w = syn.make_clips(2, 96000, seed=77)
    return cfg, emb_sd, coef, icpt, unet_sd, w, lmac_ref.explain(w, emb_sd, cfg, coef, icpt, unet_sd, audio_length=6)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_explain_pipeline_takes_six_seconds(gpu_device, precision):
    cfg, emb_sd, coef, icpt, unet_sd, w, ref = explain_setup()
    pipe = P.ExplainPipeline(cfg, emb_sd, coef, icpt, unet_sd, gpu_device, audio_length=6, precision=precision)
    out = pipe.explain(w.to(gpu_device))
    t = TOL_PIPE[precision]
    for k in ("predictions", "theta_out", "masked_predictions"):
        err = (out[k].cpu() - ref[k]).abs().max().item()
        print(f"ExplainPipeline(audio_length=6) [{precision}] {k}: max err {err:.3e}")
        assert err <= t["prob"], k
    merr = (out["mask"].cpu() - ref["mask"]).abs().max().item()
    print(f"ExplainPipeline(audio_length=6) [{precision}] mask: max err {merr:.3e}")
    assert merr <= t["mask"]
    if precision == "f32":
        assert torch.equal(out["mask"].cpu() > 0.5, ref["mask"] > 0.5)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_occlusion_and_saliency_on_six_seconds(gpu_device, precision):
    """Occlusion scores its rows through ``HipEmbedder.forward`` and takes the clip; Saliency runs the gradient chain, which names
    its limit instead of failing in the first encoder layer."""
    cfg, sd, coef, icpt = model("tiny_group")
    att = HipAttribution(embedder("tiny_group", precision))
    x = RR.clips(2, 96000, 91)
    fwd = ablation_ref.model_forward((sd, cfg, coef, icpt))
    ref, K = ablation_ref.occlusion(x, 0.0, 16000, 8000, forward=fwd)
    assert K == 11
    ours = att.occlusion(x.to(gpu_device), 16000, 8000)
    f0 = fwd(x)
    bound = 2 * TOL_LOGIT[precision] * max(1.0, f0.abs().max().item())
    err = (ours.cpu() - ref).abs().max().item()
    print(f"Occlusion 6 s [{precision}]: max |err| {err:.3e} (bound {bound:.3e}), max |attr| {ref.abs().max().item():.3e}")
    assert err <= bound
    workspaces = len(att.eg._ws)
    with pytest.raises(_lib.AdvhError, match=r"T <= 256 frames \(82319 samples\).*T = 299 \(96000 samples\).*forward-only"):
        att.saliency(x.to(gpu_device))
    assert len(att.eg._ws) == workspaces                                         # refused before any allocation
