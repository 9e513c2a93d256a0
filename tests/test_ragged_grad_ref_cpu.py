"""CPU-only: the reference the ragged gradient tests hold the kernels to (tests/ragged_grad_ref.py), pinned three ways.

1. Against central finite differences of the oracle's fp64 logit at three samples per clip (the first, the middle and the last
   valid one) with h = 1e-6: the truncation error is O(h^2) and the rounding error ~ 2^-53 |logit| / h ~ 1e-10 of a gradient
   of order one; measured <= 2.9e-9 of the clip's max|ref|, bound 1e-6.
2. For the layer-norm tiny model against autograd through HF's ``Wav2Vec2Model(attention_mask=...)`` in float64, the logit
   pooled over each clip's valid frames, as tests/test_ragged_ref_cpu.py does for the forward.  Both sides are fp64: bound 1e-9
   of the clip's max|ref| (measured in the assertion's message), and HF's gradient past a length is exactly 0.
3. That it tells the mistake apart: the padded batch differentiated as one batch of full-length clips differs from the per-clip
   gradient by more than 100 x the f32 bar of the GPU tests (1e-4) for every table length up to 2500 samples -- measured
   0.67 .. 1.06 (layer norm) and 0.99 .. 1.16 (group norm) of the clip's max|ref| at 2500, 1040, 720, 719 and 400 samples.
   The two other lengths do not show it and are not asserted: 4000 samples has nothing padded (the difference is exactly 0),
   and 3999 pads one sample, which no frame of the layer-norm model reads (7.9e-6: the normaliser alone) and which moves the
   group-norm model's statistics by 8.2e-3, under the 1e-2 asked for.
Also: the reference is exactly 0 past each length, and its logits are the forward reference's.
"""
import pytest
import torch

import ragged_grad_ref as GR
import ragged_ref as RR

MODELS = ("tiny_layer", "tiny_group")
FD_H, FD_BOUND = 1e-6, 1e-6
HF_BOUND = 1e-9
MISTAKE = 100 * 1e-4                         # 100 x the f32 bar of tests/test_gpu_ragged_grad.py
SHOWN = tuple(n for n in RR.LENGTHS if n <= 2500)


def wave():
    return RR.clips(len(RR.LENGTHS), RR.L, 91)


@pytest.mark.parametrize("name", MODELS)
def test_reference_is_zero_past_each_length_and_matches_the_forward_reference(name):
    mdl = GR.model(name)
    ref, lg = GR.input_gradient(wave(), RR.LENGTHS, mdl)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (len(RR.LENGTHS), RR.L)
    for b, n in enumerate(RR.LENGTHS):
        assert bool((ref[b, n:] == 0).all()) and ref[b, :n].abs().max() > 0
    cfg, sd, coef, icpt = mdl
    with torch.no_grad():
        fwd = RR.per_clip_classify(RR.per_clip_hidden(wave(), RR.LENGTHS, sd, cfg), coef, icpt)[0].view(-1)
    assert (lg.float() - fwd).abs().max().item() < 1e-4


@pytest.mark.parametrize("name", MODELS)
def test_reference_against_central_differences(name):
    mdl = GR.model(name)
    w = wave().double()
    ref, _ = GR.input_gradient(w, RR.LENGTHS, mdl)
    worst = 0.0
    for b, n in enumerate(RR.LENGTHS):
        for u in (0, n // 2, n - 1):
            wp, wm = w.clone(), w.clone()
            wp[b, u] += FD_H
            wm[b, u] -= FD_H
            fd = (GR.logit(wp, RR.LENGTHS, mdl)[b] - GR.logit(wm, RR.LENGTHS, mdl)[b]) / (2 * FD_H)
            e = (abs(fd - ref[b, u]) / ref[b, :n].abs().max()).item()
            print(f"{name} clip {b} ({n} samples) sample {u}: |fd - ref| / max|ref| = {e:.2e}")
            worst = max(worst, e)
    assert worst <= FD_BOUND, worst


def test_reference_against_hf_attention_mask_autograd():
    transformers = pytest.importorskip("transformers")
    from addvisor_hip import synthetic as syn
    from oracle import wav2vec2_ref
    cfg, sd, coef, icpt = mdl = GR.model("tiny_layer")
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**cfg.hf_kwargs()))
    hf.load_state_dict(syn.embedder_weights(cfg), strict=True)
    hf = hf.eval().double()
    w = wave()
    lay = RR.layer_of(cfg)
    with torch.enable_grad():
        x = w.double().requires_grad_(True)
        rows, mask = [], torch.zeros(w.shape, dtype=torch.long)
        for b, n in enumerate(RR.LENGTHS):                   # HF's feature extractor: normalised over the valid part, zeros behind
            rows.append(torch.cat([wav2vec2_ref.zero_mean_unit_var_norm(x[b:b + 1, :n])[0], x.new_zeros(RR.L - n)]))
            mask[b, :n] = 1
        hs = hf(torch.stack(rows), attention_mask=mask, output_hidden_states=True).hidden_states[lay]
        lg = GR.logits_of([hs[b, :RR.frames(cfg, n)] for b, n in enumerate(RR.LENGTHS)], coef, icpt)
        (dx,) = torch.autograd.grad(lg.sum(), x)
    ref, ref_lg = GR.input_gradient(w, RR.LENGTHS, mdl)
    errs = [e for e, _ in GR.clip_errors(dx, ref, RR.LENGTHS)]
    print("HF attention_mask autograd vs per-clip reference:", [f"{e:.1e}" for e in errs])
    assert max(errs) <= HF_BOUND, errs
    assert (lg.detach() - ref_lg).abs().max().item() <= 1e-9
    for b, n in enumerate(RR.LENGTHS):
        assert bool((dx[b, n:] == 0).all())


@pytest.mark.parametrize("name", MODELS)
def test_reference_tells_the_padded_batch_apart(name):
    mdl = GR.model(name)
    ref, _ = GR.input_gradient(wave(), RR.LENGTHS, mdl)
    pad = GR.padded_input_gradient(wave(), RR.LENGTHS, mdl)
    diff = {n: e for n, (e, _) in zip(RR.LENGTHS, GR.clip_errors(pad, ref, RR.LENGTHS))}
    print(f"{name}: padded batch vs clip alone:", {n: f"{e:.2e}" for n, e in diff.items()})
    assert SHOWN == (2500, 1040, 720, 719, 400)
    for n in SHOWN:
        assert diff[n] > MISTAKE, (n, diff[n])
    assert diff[4000] == 0.0                                 # nothing padded


@pytest.mark.parametrize("name", MODELS)
def test_layer_gradient_and_lower_vjp_compose_to_the_input_gradient(name):
    """The two halves the GPU tests use (``backward(to_layer=0)`` and ``backward(from_layer=0, layer_seed=S)``) chain to the whole."""
    cfg = (mdl := GR.model(name))[0]
    w = wave()
    g0 = GR.layer_gradient(w, RR.LENGTHS, mdl, 0)
    T = RR.frames(cfg, RR.L)
    S = torch.zeros(len(RR.LENGTHS), T, cfg.hidden_size, dtype=torch.float64)
    for b, g in enumerate(g0):
        assert g.shape[0] == RR.frames(cfg, RR.LENGTHS[b])
        S[b, :g.shape[0]] = g
    dx = GR.lower_vjp(w, RR.LENGTHS, mdl, S)
    ref, _ = GR.input_gradient(w, RR.LENGTHS, mdl)
    assert max(e for e, _ in GR.clip_errors(dx, ref, RR.LENGTHS)) <= 1e-10
