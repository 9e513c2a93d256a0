"""GPU: ``HipSpectralAttribution.optimize_mask`` (addvisor_hip/mask_opt.py; csrc/mask_opt.hip around the forward / backward chain
and the row-mapped ISTFT pair) against the float64 restatement of tests/mask_opt_ref.py driven by the oracle's model
(``spectral_attr_ref.MaskModel``).

The fixtures are those of tests/test_gpu_spectral_attr.py, re-declared: ``tiny_config``, B = 2, L = 16000 (T = 50), the crop
(512, 48) and the full (513, 50), both domains.  Every call uses ``cell = (64, 8)`` (grids (8, 6) and (9, 7): the restatement
stays cheap), ``area = 0.25``, every lambda non-zero, ``init_noise = 0.1`` with a fixed seed (no ties)."""
import pytest
import torch
import torch.nn.functional as F

import mask_opt_ref as R
import spectral_attr_ref as SR
from addvisor_hip import mask_opt as MO, ops, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.spectral_attribution import HipSpectralAttribution

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}                  # tests/test_gpu_spectral_attr.py
B, L, T = 2, 16000, 50
CROPS = [(512, 48), (513, 50)]
CROP_IDS = ["crop", "full"]
DOMAINS = ["linear", "log1p"]
LAM = dict(lam_in=1.0, lam_out=1.0, lam_area=1.0, lam_l1=0.05, lam_tv=0.1)
COMMON = dict(area=0.25, cell=(64, 8), init=0.5, init_noise=0.1, seed=3, **LAM)
LAM_T = tuple(LAM.values())
SGD_LR = 2.0

_ATT, _ENG, _MM = {}, {}, {}


def clips():
    return syn.make_clips(B, L, seed=12)


def model():
    if "model" not in _ATT:
        cfg = syn.tiny_config(False)
        _ATT["model"] = (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))
    return _ATT["model"]


def attribution(dev, precision, **kw):
    key = (precision,) + tuple(kw.items())
    if key not in _ATT:
        sd, cfg, coef, icpt = model()
        _ATT[key] = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision), **kw)
    return _ATT[key]


def engine(dev, precision="f32", domain="linear"):
    if (precision, domain) not in _ENG:
        _ENG[precision, domain] = HipSpectralAttribution(attribution(dev, precision), clips().to(dev), domain)
    return _ENG[precision, domain]


def restatement(domain="linear"):
    if domain not in _MM:
        _MM[domain] = SR.MaskModel(clips(), model(), domain)
    return _MM[domain]


def checked(crop, domain="linear", **kw):
    """The normalised arguments of a call (``K1``, the start theta) for the restatement."""
    return MO.check_mask_opt_args(B, T, domain, shape=crop, **{**COMMON, **kw})


def relerr(a, b):
    return ((a.cpu().double() - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_teacher_forced_gradient_parity(gpu_device, precision, domain, crop):
    """Four Adam steps with ``trace``: at every traced theta_k the restatement's ``grad_theta`` against the device's, at the
    project's method bars (f32: 1e-4 of max |ref|, cosine 0.999999; f16: 3e-2, 0.999) -- one-step comparisons at visited points,
    so no trajectory divergence accumulates."""
    eng, mm, a = engine(gpu_device, precision, domain), restatement(domain), checked(crop, domain)
    trace = []
    res = eng.optimize_mask(steps=4, shape=crop, trace=trace, **COMMON)
    assert len(trace) == 4 and torch.equal(trace[0][0].cpu(), a.theta0)
    tol, cmin = TOL[precision]
    sign = res.sign.cpu().double()
    assert sign.tolist() == torch.where(mm.logit(torch.ones(B, *crop)) >= 0, 1.0, -1.0).tolist()
    for k, (theta_k, grad_k, logits_k, seeds_k) in enumerate(trace):
        ref, rseeds, rlogits, _ = R.model_step(mm, theta_k.cpu(), sign, LAM_T, a.K1, "log_prob", *crop)
        err = relerr(grad_k, ref)
        cos = F.cosine_similarity(grad_k.cpu().double().flatten(), ref.flatten(), dim=0).item()
        print(f"step {k} [{precision}, {domain}, {crop}]: grad_theta max rel err {err:.3e}, cosine {cos:.8f}; "
              f"logits {relerr(logits_k, rlogits):.3e}, seeds {relerr(seeds_k, rseeds):.3e}")
        assert tuple(grad_k.shape) == (B, a.Fc, a.Tc) and tuple(logits_k.shape) == tuple(seeds_k.shape) == (2 * B,)
        assert err < tol and cos > cmin, (k, err, cos)
    assert not torch.equal(trace[1][0], trace[0][0])
    assert all(tuple(v.shape) == (4, B) for v in res.history.values()) and list(res.history) == list(MO.HISTORY)


@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_free_running_sgd_trajectory(gpu_device, precision, domain, crop):
    """SGD with momentum 0, 5 steps at lr = 2, against the restatement's own 5 steps: ``max |dtheta - dtheta_ref| / max
    |dtheta_ref|`` (``dtheta`` = theta after 5 steps - the start) is printed and held to the teacher-forced bar times the step
    count, a first-order bound."""
    eng, mm, a = engine(gpu_device, precision, domain), restatement(domain), checked(crop, domain)
    res = eng.optimize_mask(steps=5, shape=crop, optimizer="sgd", momentum=0.0, lr=SGD_LR, **COMMON)
    thetas, _ = R.sgd_run(mm, a.theta0, res.sign.cpu().double(), LAM_T, a.K1, "log_prob", *crop, SGD_LR, 5)
    d_ref = thetas[-1] - a.theta0.double()
    d_dev = res.theta.cpu().double() - a.theta0.double()
    err = ((d_dev - d_ref).abs().max() / d_ref.abs().max()).item()
    print(f"free-running SGD [{precision}, {domain}, {crop}]: max |dtheta - ref| / max |ref| = {err:.3e}")
    assert err < 5 * TOL[precision][0]


@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_sgd_descends(gpu_device, crop):
    """SGD with momentum 0, 8 steps at lr = 2 in the ``linear`` domain: on the CPU the restatement's ``J_b`` falls at every step
    for both clips at this lr (by 0.02 or more a step, asserted here too; at lr = 10 it does not), and the device history's must
    as well.  fp32-class chain: the fall per step is far above its noise."""
    eng, mm, a = engine(gpu_device, "f32", "linear"), restatement("linear"), checked(crop)
    res = eng.optimize_mask(steps=8, shape=crop, optimizer="sgd", momentum=0.0, lr=SGD_LR, **COMMON)
    _, hist = R.sgd_run(mm, a.theta0, res.sign.cpu().double(), LAM_T, a.K1, "log_prob", *crop, SGD_LR, 8)
    J_ref, J = hist[:, :, 5], res.history["objective"].cpu().double()
    print(f"J ref {J_ref.T.tolist()}\nJ dev {J.T.tolist()}")
    assert bool((J_ref[1:] < J_ref[:-1]).all()), "the restatement itself must descend at this lr"
    assert bool((J[1:] < J[:-1]).all())


def test_bit_identity_and_chunking(gpu_device):
    """A second call, ``internal_batch_size`` 2 against 4 (one clip and two clips per chunk), and clip 0 of the 2-clip engine
    against a 1-clip engine over that clip: the same bits."""
    eng = engine(gpu_device)
    kw = dict(steps=3, shape=CROPS[1], **COMMON)
    first = eng.optimize_mask(internal_batch_size=4, **kw)
    for other in (eng.optimize_mask(internal_batch_size=4, **kw), eng.optimize_mask(internal_batch_size=2, **kw), eng.optimize_mask(**kw)):
        assert torch.equal(first.theta, other.theta) and torch.equal(first.mask, other.mask)
        assert all(torch.equal(first.history[k], other.history[k]) for k in MO.HISTORY)
        assert torch.equal(first.logits_in, other.logits_in) and torch.equal(first.logits_out, other.logits_out)
    a = checked(CROPS[1])
    one = HipSpectralAttribution(attribution(gpu_device, "f32"), clips()[:1].to(gpu_device), "linear")
    solo = one.optimize_mask(**{**kw, "init": torch.sigmoid(a.theta0[:1].double()), "init_noise": 0.0})
    assert (solo.theta.cpu() - a.theta0[:1]).abs().max() > 0.01            # it moved
    # theta0 of the solo run is logit(sigmoid(theta0)) in float64 rounded to fp32: equal to the 2-clip start bit for bit
    assert torch.equal(MO.check_mask_opt_args(1, T, "linear", shape=CROPS[1], **{**COMMON, "init": torch.sigmoid(a.theta0[:1].double()),
                                                                                   "init_noise": 0.0}).theta0, a.theta0[:1])
    assert torch.equal(solo.theta, first.theta[:1]) and torch.equal(solo.mask, first.mask[:1])


@pytest.mark.parametrize("domain", DOMAINS)
def test_the_result_is_consistent(gpu_device, domain):
    """``mask`` is bitwise the rows kernel of ``theta``; ``logits_in`` / ``logits_out`` are ``engine.logits`` of the mask and of
    its complement; ``coarse``, ``area_reached`` and ``logit`` are what they say."""
    eng, crop = engine(gpu_device, "f32", domain), CROPS[0]
    res = eng.optimize_mask(steps=3, shape=crop, **COMMON)
    a = checked(crop, domain)
    rows = MO.mask_rows(a.desc(), res.theta, 0, B)
    assert torch.equal(res.mask, rows[0::2].view(B, *crop))
    assert torch.equal(res.logits_in, eng.logits(res.mask)) and torch.equal(res.logits_out, eng.logits(1.0 - res.mask))
    assert torch.equal(res.logit, eng.logits(torch.ones((B,) + crop, device=gpu_device)))
    assert torch.equal(res.coarse, MO.coarse_of(res.theta)) and tuple(res.coarse.shape) == (B, a.Fc, a.Tc)
    assert (res.coarse.cpu().double() - torch.sigmoid(res.theta.cpu().double())).abs().max() < 1e-6
    assert torch.equal(res.area_reached, (res.coarse > 0.5).float().flatten(1).mean(1))
    assert bool(torch.isfinite(res.mask).all()) and float(res.mask.min()) >= 0 and float(res.mask.max()) <= 1
    with_target = eng.optimize_mask(steps=1, shape=crop, target=torch.tensor([0, 0]), **COMMON)
    assert with_target.sign.tolist() == [-1.0, -1.0]


class _Wave:
    """The waveform model of the front end, on the tiny embedder."""
    def __init__(self, att):
        self._att = att

    def hip_attribution(self):
        return self._att


def test_explain_spectrogram_optimized_mask(gpu_device):
    """Three finite ``[B, 1]`` tensors: one forward over the clip and the two ``log1p`` resyntheses of the optimised mask."""
    import captum_saliency as CS
    att = attribution(gpu_device, "f32")
    x = clips().to(gpu_device)
    opt = dict(steps=3, **COMMON)
    out = CS.explain_spectrogram(_Wave(att), x, "optimized_mask", mask=torch.ones(B, *CROPS[0]), mask_opt=opt)
    assert all(tuple(o.shape) == (B, 1) and bool(torch.isfinite(o).all()) for o in out)
    res = engine(gpu_device).optimize_mask(shape=CROPS[0], **opt)
    w_in, w_out = ops.istft_masked_c64(engine(gpu_device).spec, res.mask, L, "log1p")
    p = att.emb.forward(torch.cat([x, w_in, w_out]), want_hidden=False)[2]
    for o, want in zip(out, (p[:B], p[B:2 * B], p[2 * B:])):
        assert torch.equal(o, want)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_a_saturated_seed_raises(gpu_device, precision):
    """``lam_in`` far beyond the range ``loss_scale`` leaves (the seed times the scale overflows the chain's planes): an
    arithmetic overflow, reported as FloatingPointError naming ``loss_scale`` instead of a poisoned mask."""
    eng = engine(gpu_device, precision)
    with pytest.raises(FloatingPointError, match="loss_scale"):
        eng.optimize_mask(steps=2, shape=CROPS[0], **{**COMMON, "lam_in": 1e30, "reward": "logit"})
    res = eng.optimize_mask(steps=1, shape=CROPS[0], **COMMON)             # the engine is usable afterwards
    assert bool(torch.isfinite(res.theta).all())
