"""GPU: ``ExplainPipeline.explain(waves, lengths=...)`` on the shared length table of tests/ragged_explain_ref.py, both precisions
and both mask domains: against the per-clip-alone oracle at the bars of tests/test_gpu_pipeline.py, exact zeros past every clip's
extent, garbage past the lengths without effect, full lengths equal to the padded call bit for bit, every clip against the
existing engine on the cropped clip alone, a batch beyond 256 frames, the LMAC metrics of the ragged probabilities, the host-side
refusals, and ``LMAC_metrics.explain_batch(..., lengths=)``."""
import os

import pytest
import torch

import ragged_explain_ref as E
from addvisor_hip import pipeline as P, runtime, synthetic as syn
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.unet import HipUNet
from oracle import lmac_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LENS, B = list(E.LENGTHS), len(E.LENGTHS)
BOTH = [(p, d) for p in ("f32", "f16") for d in ("log1p", "linear")]
KEEP = ("spec", "mag", "mask", "wave_in", "wave_out") + E.PROBS


@pytest.fixture(scope="module")
def engines(gpu_device):
    """One embedder and one U-Net per precision, shared by every pipeline of this file."""
    cache = {}

    def get(precision):
        if precision not in cache:
            cfg, emb_sd, unet_sd, coef, icpt = E.models()
            cache[precision] = (HipEmbedder(cfg, emb_sd, coef, icpt, gpu_device, precision=precision),
                                HipUNet(unet_sd, gpu_device, precision=precision))
        return cache[precision]
    return get


def pipe_of(engines, dev, precision, domain, samples=E.L):
    emb, unet = engines(precision)
    return P.ExplainPipeline(None, None, None, None, None, dev, audio_length=samples, sampling_rate=1, domain=domain,
                             precision=precision, embedder=emb, unet=unet)


def same_bits(a, b):
    return all(torch.equal(torch.view_as_real(a[k]) if a[k].is_complex() else a[k], torch.view_as_real(b[k]) if b[k].is_complex() else b[k])
               for k in KEEP)


def check_vs_oracle(out, ref, lens, precision, tag):
    t = E.TOL[precision]
    for k in E.PROBS:
        err = (out[k].cpu() - ref[k]).abs().max().item()
        print(f"{tag} {k}: max |err| vs the clip alone = {err:.3e} (bar {t['prob']:.0e})")
        assert err <= t["prob"], (tag, k, err)
    merr = (out["mask"].cpu() - ref["mask"]).abs().max().item()
    werr = max((out[k].cpu() - ref[k]).abs().max().item() for k in ("wave_in", "wave_out"))
    print(f"{tag} mask {merr:.3e} (bar {t['mask']:.1e}), waves {werr:.3e} (bar {t['wave']:.0e})")
    assert merr <= t["mask"] and werr <= t["wave"], (tag, merr, werr)
    if precision == "f32":
        assert torch.equal(out["mask"].cpu() > 0.5, ref["mask"] > 0.5)
    for b, n in enumerate(lens):                                                 # every zero region exactly 0
        Tb, Wb = E.frame_counts(n)
        assert (torch.view_as_real(out["spec"][b, :, Tb:]) == 0).all() and (out["mag"][b, :, Tb:] == 0).all(), (tag, b)
        assert (out["mask"][b, :, Wb:] == 0).all(), (tag, b)
        assert (out["wave_in"][b, n:] == 0).all() and (out["wave_out"][b, n:] == 0).all(), (tag, b)


@pytest.mark.parametrize("precision,domain", BOTH)
def test_table_vs_oracle_zero_regions_and_garbage(gpu_device, engines, precision, domain):
    pipe = pipe_of(engines, gpu_device, precision, domain)
    w = E.clips().to(gpu_device)
    out = pipe.explain(w, keep=True, lengths=LENS)
    check_vs_oracle(out, E.table_reference(domain), LENS, precision, f"[{precision} {domain}]")
    for junk in (float("nan"), 1e30):                                            # what lies past a clip's length changes no bit
        wj = w.clone()
        for b, n in enumerate(LENS):
            wj[b, n:] = junk
        assert same_bits(pipe.explain(wj, keep=True, lengths=torch.tensor(LENS)), out), (precision, domain, junk)
    wide = torch.cat([w, torch.full((B, 37), float("nan"), device=gpu_device)], 1)      # columns past the buffer are not read either
    assert same_bits(pipe.explain(wide, keep=True, lengths=LENS), out)


@pytest.mark.parametrize("precision,domain", BOTH)
def test_full_lengths_equal_the_padded_call(gpu_device, engines, precision, domain):
    pipe = pipe_of(engines, gpu_device, precision, domain)
    w = E.clips().to(gpu_device)
    assert same_bits(pipe.explain(w, keep=True, lengths=[E.L] * B), pipe.explain(w, keep=True))


@pytest.mark.parametrize("precision,domain", BOTH)
def test_each_clip_against_the_engine_on_the_cropped_clip_alone(gpu_device, engines, precision, domain):
    """The existing engine, ``B = 1``, an audio length of exactly ``n_b`` samples, the same embedder and U-Net: bit for bit in the
    fp32-class mode, the same probabilities to the fp16 bar in fp16 mode."""
    pipe = pipe_of(engines, gpu_device, precision, domain)
    w = E.clips().to(gpu_device)
    out = pipe.explain(w, keep=True, lengths=LENS)
    for b, n in enumerate(LENS):
        Tb, Wb = E.frame_counts(n)
        alone = pipe_of(engines, gpu_device, precision, domain, samples=n).explain(w[b:b + 1, :n].contiguous(), keep=True)
        crop = dict(spec=out["spec"][b:b + 1, :, :Tb], mag=out["mag"][b:b + 1, :, :Tb], mask=out["mask"][b:b + 1, :, :Wb],
                    wave_in=out["wave_in"][b:b + 1, :n], wave_out=out["wave_out"][b:b + 1, :n], **{k: out[k][b:b + 1] for k in E.PROBS})
        diff = {k: (alone[k] - crop[k]).abs().max().item() for k in KEEP}
        print(f"[{precision} {domain}] clip {b} ({n} samples): alone vs ragged batch " + ", ".join(f"{k} {v:.1e}" for k, v in diff.items()))
        if precision == "f32":
            assert same_bits(alone, crop), (b, n, diff)
        else:
            assert all(diff[k] <= E.TOL["f16"]["prob"] for k in E.PROBS), (b, n, diff)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_long_batch_vs_oracle(gpu_device, engines, precision):
    """83 200, 40 000 and 966 samples in one buffer: 259 frames, past the whole-clip attention's 256."""
    w, ref = E.long_reference()
    pipe = pipe_of(engines, gpu_device, precision, "log1p", samples=E.LONG_L)
    assert pipe.frame_counts(E.LONG_LENGTHS) == ([259, 125, 4], [256, 124, 4])
    out = pipe.explain(w.to(gpu_device), keep=True, lengths=list(E.LONG_LENGTHS))
    check_vs_oracle(out, ref, E.LONG_LENGTHS, precision, f"[{precision} long]")


def test_lmac_metrics_of_the_ragged_probabilities(gpu_device, engines):
    pipe = pipe_of(engines, gpu_device, "f32", "log1p")
    out = pipe.explain(E.clips().to(gpu_device), lengths=LENS)
    got, pc = P.lmac_metrics(out["predictions"], out["theta_out"], out["masked_predictions"], per_clip=True)
    p, t, o = (out[k].cpu() for k in E.PROBS)
    mine = lmac_ref.lmac_summary(p, t, o)                                        # the reference's metric functions on the same probabilities
    for k in mine:
        assert abs(got[k] - mine[k]) <= 1e-5 * max(1.0, abs(mine[k])), (k, got[k], mine[k])
    pc = pc.cpu()
    assert torch.equal(pc[0], lmac_ref.compute_faithfulness(p, o)) and torch.equal(pc[1], lmac_ref.compute_fidelity(t, p).view(-1))
    assert torch.allclose(pc[2], lmac_ref.compute_AD(t, p), rtol=1e-6, atol=1e-6) and torch.equal(pc[3], lmac_ref.compute_AI(t, p))
    ref = E.table_reference()
    oracle = lmac_ref.lmac_summary(ref["predictions"], ref["theta_out"], ref["masked_predictions"])
    print("ragged metrics", got, "oracle, every clip alone", oracle)
    assert abs(got["faithfulness"] - oracle["faithfulness"]) <= 2 * E.TOL["f32"]["prob"] and abs(got["fidelity"] - oracle["fidelity"]) <= 1e-6


def test_refusals_happen_before_any_launch(gpu_device, engines):
    pipe = pipe_of(engines, gpu_device, "f32", "log1p")
    emb, unet = engines("f32")
    w = E.clips()[:2].to(gpu_device)
    before = (set(emb._ws), set(unet._ws))                                       # a batch of two has no workspace yet: none may appear
    assert not any(k[0] == 2 for k in before[1]) and not any(k[0] in (2, 6) for k in before[0])
    for bad, msg in (([8000, 965], r"clip 1 has 965 samples.*shortest supported length is 966"), ([8001, 8000], r"lengths\[0\] = 8001 exceeds"),
                     ([8000], "1 entries for a batch of 2"), ([8000, 966.0], "not an integer"), ([8000, True], "not an integer"),
                     (torch.tensor([8000.0, 966.0]), "integer tensor"), (5, "integer tensor")):
        with pytest.raises(ValueError, match=msg):
            pipe.explain(w, lengths=bad)
    with pytest.raises(ValueError, match="columns"):
        pipe.explain(w[:, :7000].contiguous(), lengths=[8000, 966])
    with pytest.raises(ValueError, match="CUDA fp32"):
        pipe.explain(w.double(), lengths=[8000, 966])
    voc = pipe_of(engines, gpu_device, "f32", "log1p")
    voc.vocoder = object()                                                       # refused before it is ever called
    with pytest.raises(ValueError, match="vocoder"):
        voc.explain(w, lengths=[8000, 966])
    assert (set(emb._ws), set(unet._ws)) == before
    assert pipe.min_length() == 966


def test_explain_batch_with_lengths(gpu_device):
    """The drop-in module's fused step takes ``lengths``: the same call on its own pipeline, and the oracle on each clip alone."""
    import LMAC_metrics
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    LMAC_metrics._model = None
    LMAC_metrics._pipes.clear()
    old = LMAC_metrics.audio_processor.audio_length
    LMAC_metrics.audio_processor.audio_length = E.L / 16000
    try:
        import audioprocessor
        clips = [E.clips()[b, :n] for b, n in ((0, 8000), (4, 6440), (8, 966))]
        waves, lens = audioprocessor.pad_clips(clips)
        got = LMAC_metrics.explain_batch(waves, lengths=lens)
        direct = LMAC_metrics._pipeline().explain(waves.to(gpu_device), lengths=lens)
        assert all(g.shape == (3, 1) for g in got) and all(torch.equal(g, direct[k]) for g, k in zip(got, E.PROBS))
        cfg, sd = runtime.embedder_config_and_weights()
        clf = runtime.classifier()
        ref = E.explain_ragged(waves, lens, weights=(cfg, sd, syn.unet_weights(), clf.coef_, clf.intercept_))
        tol = E.TOL[runtime.hip_embedder().precision]["prob"]
        for g, k in zip(got, E.PROBS):
            assert (g.cpu() - ref[k]).abs().max().item() <= tol, k
        with pytest.raises(ValueError, match="explicit magnitude"):
            LMAC_metrics.explain_batch(waves, magnitude=torch.zeros(3, 513, 25), lengths=lens)
    finally:
        LMAC_metrics.audio_processor.audio_length = old
        LMAC_metrics._model = None
        LMAC_metrics._pipes.clear()
        os.environ.pop("ADDVISOR_EMBEDDER", None)
        runtime.reset()
