"""``HipAttribution.saliency / input_x_gradient / integrated_gradients(..., lengths=...)`` on the ragged batch of
tests/ragged_ref.py (seven lengths at L = 4000), tiny layer-norm and group-norm models, both precisions.

Each result is compared per clip with the same method called on the cropped clip alone (no lengths, B = 1) and with
oracle/attribution_ref.py on the cropped clip, at the bars of tests/test_gpu_attribution_baselines.py (f32 1e-4 of the clip's
max|ref| and cosine > 0.999999; f16 3e-2 and 0.999; deltas within ``DELTA_TOL``); values past a length are exactly 0; the
result does not depend on ``internal_batch_size``, bit for bit.  Where the EXISTING engine on the cropped clip alone measures
above a bar against the oracle, that case's bar is twice the measurement (``PARENT_BAR``)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import ragged_grad_ref as GR
import ragged_ref as RR
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from oracle import attribution_ref
from test_gpu_attribution_baselines import DELTA_TOL, TOL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CASES = [(n, p) for n in ("tiny_layer", "tiny_group") for p in ("f32", "f16")]
N_STEPS, TWO_CHUNKS = 4, 14                               # 7 clips x 4 steps = 28 rows: 14 rows per chunk = two chunks of two steps
# (model, precision, method, samples) -> (error bar, cosine bar): twice the existing engine's own measurement on that clip alone
PARENT_BAR = {}


@functools.lru_cache(maxsize=None)
def engine(name, precision):
    cfg, sd, coef, icpt = GR.model(name)
    return HipAttribution(HipEmbedder(cfg, sd, coef, icpt, torch.device("cuda:0"), precision=precision))


@functools.lru_cache(maxsize=None)
def oracle(name, method):
    """Per clip, on the cropped clip alone.  Shared: never modify."""
    cfg, sd, coef, icpt = GR.model(name)
    wave = RR.clips(len(RR.LENGTHS), RR.L, 91)
    fn = {"saliency": attribution_ref.saliency, "ixg": attribution_ref.input_x_gradient,
          "ig": functools.partial(attribution_ref.integrated_gradients, n_steps=N_STEPS)}[method]
    with torch.enable_grad():
        return [fn(wave[b:b + 1, :n].contiguous(), sd, cfg, coef, icpt)[0] for b, n in enumerate(RR.LENGTHS)]


def errors(got, ref):
    g, r = got.double().cpu().flatten(), ref.double().flatten()
    return ((g - r).abs().max() / (r.abs().max() + 1e-30)).item(), F.cosine_similarity(g, r, dim=0).item()


def garbage(wave, value):
    w = wave.clone()
    for b, n in enumerate(RR.LENGTHS):
        w[b, n:] = value
    return w


@pytest.mark.parametrize("name,precision", CASES)
def test_ragged_attributions(gpu_device, name, precision):
    att = engine(name, precision)
    wave = RR.clips(len(RR.LENGTHS), RR.L, 91)
    w = garbage(wave, 1e30).to(gpu_device)                  # the padding is never read for its value
    lengths = list(RR.LENGTHS)
    sal = att.saliency(w, lengths=lengths)
    ixg = att.input_x_gradient(w, lengths=torch.tensor(lengths))
    ig, delta = att.integrated_gradients(w, n_steps=N_STEPS, internal_batch_size=TWO_CHUNKS, return_convergence_delta=True, lengths=lengths)
    assert delta.shape == (len(lengths),)
    fx, f0 = att.logits(w, lengths=lengths).double().cpu(), att.logits(torch.zeros_like(w), lengths=lengths).double().cpu()
    mine = ig.double().cpu().sum(1) - (fx - f0)
    print(f"{name} [{precision}] delta {delta.tolist()} vs sum(attr) - (F(x) - F(0)) from the ragged forward {mine.tolist()}")
    assert (delta.double().cpu() - mine).abs().max().item() < 1e-5     # the delta's F is the ragged forward
    rel, ab = DELTA_TOL[precision]
    rows = []
    for b, n in enumerate(lengths):
        x1 = wave[b:b + 1, :n].contiguous().to(gpu_device)
        ig1, d1 = att.integrated_gradients(x1, n_steps=N_STEPS, return_convergence_delta=True)
        for method, got, one in (("saliency", sal, att.saliency(x1)), ("ixg", ixg, att.input_x_gradient(x1)), ("ig", ig, ig1)):
            assert bool((got[b, n:] == 0).all()), (method, b, "values past the clip's length are not exactly zero")
            ref = oracle(name, method)[b]
            e, c = errors(got[b, :n], ref)
            e1, c1 = errors(one[0], ref)
            ea, _ = errors(got[b, :n], one[0].cpu())
            same = torch.equal(got[b, :n], one[0])
            print(f"{name} [{precision}] {method} clip {b} ({n} samples): vs oracle err {e:.3e} cosine {c:.8f} | the engine alone vs oracle "
                  f"err {e1:.3e} cosine {c1:.8f} | vs the engine alone err {ea:.3e} bit-identical {same}")
            rows.append((method, n, e, c, ea))
        dd = abs(delta[b].item() - d1[0].item())
        print(f"{name} [{precision}] delta clip {b} ({n} samples): {delta[b].item():.6e} | alone {d1[0].item():.6e}")
        assert dd <= rel * abs(fx[b].item() - f0[b].item()) + ab, (b, n, dd)
    for method, n, e, c, ea in rows:
        tol, cmin = PARENT_BAR.get((name, precision, method, n), TOL[precision])
        assert e < tol and c > cmin, (name, precision, method, n, e, c)
        assert ea < TOL[precision][0], (name, precision, method, n, ea)


@pytest.mark.parametrize("name,precision", CASES)
def test_internal_batch_size_changes_no_bit(gpu_device, name, precision):
    att = engine(name, precision)
    w = RR.clips(len(RR.LENGTHS), RR.L, 91).to(gpu_device)
    lengths = list(RR.LENGTHS)
    ref = att.integrated_gradients(w, n_steps=N_STEPS, return_convergence_delta=True, lengths=lengths)
    for ibs in (7, TWO_CHUNKS, 21):                          # one step per chunk, two, three (a padded last chunk)
        got = att.integrated_gradients(w, n_steps=N_STEPS, internal_batch_size=ibs, return_convergence_delta=True, lengths=lengths)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), ibs
    plain = att.integrated_gradients(w, n_steps=N_STEPS, multiply_by_inputs=False, lengths=lengths)
    assert all(bool((plain[b, n:] == 0).all()) for b, n in enumerate(lengths))
    # the seam without lengths is as it was: same bits as before and after a ragged call
    a = att.saliency(w)
    att.saliency(w, lengths=lengths)
    assert torch.equal(att.saliency(w), a) and att._lens is None


def test_nonzero_baselines_carry_the_lengths(gpu_device):
    """A ``[1, L]`` and a ``[B, L]`` baseline: zero past each length like the input, F(baseline) under each clip's own length."""
    att = engine("tiny_layer", "f32")
    wave = RR.clips(len(RR.LENGTHS), RR.L, 91)
    w, lengths = wave.to(gpu_device), list(RR.LENGTHS)
    base = 0.05 * torch.randn(1, RR.L, generator=torch.Generator().manual_seed(3))
    a1, d1 = att.integrated_gradients(w, n_steps=N_STEPS, baselines=base.to(gpu_device), return_convergence_delta=True, lengths=lengths)
    aB, dB = att.integrated_gradients(w, n_steps=N_STEPS, baselines=base.expand(len(lengths), RR.L).contiguous().to(gpu_device),
                                      return_convergence_delta=True, lengths=lengths)
    assert torch.equal(a1, aB) and torch.equal(d1, dB)
    for b, n in enumerate(lengths):
        x1, b1 = wave[b:b + 1, :n].contiguous().to(gpu_device), base[:, :n].contiguous().to(gpu_device)
        one, dd = att.integrated_gradients(x1, n_steps=N_STEPS, baselines=b1, return_convergence_delta=True)
        e, _ = errors(a1[b, :n], one[0].cpu())
        print(f"IG with a noise baseline, clip {b} ({n} samples): vs the engine alone err {e:.3e}, delta {d1[b].item():.4e} | {dd[0].item():.4e}")
        assert e < TOL["f32"][0] and bool((a1[b, n:] == 0).all())
        assert abs(d1[b].item() - dd[0].item()) <= 1e-3 * abs(d1[b].item()) + 1e-4
