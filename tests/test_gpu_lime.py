"""GPU: Lime and FeaturePermutation on csrc/attribution_lime.hip and the HIP forward, against the Captum-style restatement of
tests/lime_ref.py: the permuted rows bit for bit, the similarity weights against the float64 kernel, Lime's fit on the engine's
own logits and on the oracle's, FeaturePermutation on the oracle's logits, chunking and seeds, the captum.attr front end, and the
integration with NoiseTunnel, explain_waves and score_explanations."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import lime_ref as R
from addvisor_hip import attribution as AT, linear_model as LM, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}          # the stated logit parities
U32 = 2.0 ** -24                                # fp32 unit roundoff

_CACHE = {}


def setup(dev, precision):
    if precision not in _CACHE:
        cfg = syn.tiny_config(False)
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[precision] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[precision]


def noise(B, L, seed):
    return 0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def misaligned(t):
    """A contiguous copy of ``t`` whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def segments(L, K, B=1):
    return (torch.arange(L) * K // L)[None].expand(B, L).contiguous()


def refit(model, z, y, w):
    model.fit(DataLoader(TensorDataset(torch.from_numpy(z.astype(np.float32)), torch.from_numpy(np.ascontiguousarray(y)),
                                       torch.from_numpy(np.ascontiguousarray(w))), batch_size=len(y)))
    return model.representation().numpy().reshape(-1)


def test_permuted_rows_equal_the_restatement(gpu_device):
    dev = gpu_device
    B, K = 3, 5
    for L in (1000, 1001):                                               # float4 and scalar forms
        x = syn.make_clips(B, L, seed=L)
        index = torch.randint(0, K, (1, L), generator=torch.Generator().manual_seed(L), dtype=torch.int32)
        perm = AT.feature_permutation_draws(L, K, B)
        ref = torch.from_numpy(R.permuted_rows(x.numpy(), index.numpy(), perm))
        for view in ("aligned", "misaligned"):
            xd = x.to(dev) if view == "aligned" else misaligned(x.to(dev))
            idd, pd = index.to(dev), torch.from_numpy(perm).to(dev)
            d = AT.permutation_desc(xd, idd, pd)
            out = torch.full((K * B, L), float("nan"), device=dev)
            AT.permutation_points(d, 0, K * B, out)
            assert torch.equal(out.cpu(), ref), (L, view)
            chunked = torch.full((K * B, L), float("nan"), device=dev)       # the engine's chunks: a padded last one
            work = torch.full((4, L), float("nan"), device=dev)
            for row0 in range(0, K * B, 4):
                AT.permutation_points(d, row0, 4, work)
                n = min(4, K * B - row0)
                chunked[row0:row0 + n] = work[:n]
                if n < 4:                                                # rows past K * B copy x[g % B]
                    assert torch.equal(work[n:].cpu(), x[[(K * B + i) % B for i in range(4 - n)]]), (L, view)
            assert torch.equal(chunked.cpu(), ref), (L, view)


def test_row_similarity_against_float64(gpu_device):
    dev = gpu_device
    B, S, K = 3, 4, 6
    for L in (1000, 1001):
        x = syn.make_clips(B, L, seed=L + 1)
        base = noise(1, L, 3) + 0.01                                     # a non-zero baseline
        index = segments(L, K)
        z = AT.lime_draws(L, [K] * B, S)
        rows = torch.stack([R.kernel_shap_rows(x, base, index[0], z[b], b)[s] for s in range(S) for b in range(B)])   # s * B + b
        rows[4] = 0                                                      # an all-zero row: cos = 0
        n = S * B
        got = {}
        for mode, width in (("cosine", 1.0), ("cosine", 0.25), ("euclidean", 9.0)):
            want = np.array([R.similarity(x[g % B], rows[g], mode, width) for g in range(n)])
            for view in ("aligned", "misaligned"):
                put = (lambda t: t.to(dev)) if view == "aligned" else (lambda t: misaligned(t.to(dev)))
                xd, rd = put(x), put(rows)
                sim = torch.full((n,), float("nan"), device=dev)
                AT.row_similarity(rd, xd, 0, n, AT.SIM_MODES.index(mode), width, sim)
                s = sim.cpu().double().numpy()
                err = np.abs(s - want) / want
                print(f"row similarity L = {L} {mode} w = {width} [{view}]: max rel err {err.max():.3e}, weights {s.min():.3e}..{s.max():.3e}")
                assert np.all(err <= 1e-6), (L, mode, view)
                chunked = torch.full((n,), float("nan"), device=dev)     # 5-row chunks, the last one padded: same bits
                work = torch.zeros((5, L), device=dev)
                for row0 in range(0, n, 5):
                    m = min(5, n - row0)
                    work[:m] = rd[row0:row0 + m]
                    AT.row_similarity(work, xd, row0, m, AT.SIM_MODES.index(mode), width, chunked)
                assert torch.equal(chunked, sim), (L, mode, view)
                got[view] = sim.cpu()
            if L == 1000:
                assert torch.equal(got["aligned"], got["misaligned"])     # float4 and scalar paths: the same order


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_lime_against_its_own_logits_and_the_oracle(gpu_device, precision):
    dev = gpu_device
    att, model = setup(dev, precision)
    B, L, S = 2, 16000, 40
    x = syn.make_clips(B, L, seed=61)
    base = noise(1, L, 12)
    mask = torch.stack([segments(L, 6)[0] * 2 - 5, segments(L, 8)[0] + 3])  # different features per clip, negative ids too
    index, Ks = AT.per_clip_feature_indices(mask, B, L)
    assert Ks == [6, 8]
    z = AT.lime_draws(13, Ks, S)
    rows = [R.kernel_shap_rows(x, base, index[b], z[b], b) for b in range(B)]
    y_oracle = [R.model_forward(model)(rows[b]).double().numpy() for b in range(B)]
    w64 = np.array([[R.similarity(x[b], rows[b][s], "cosine", 1.0) for b in range(B)] for s in range(S)])
    for alpha in (0.01, 1e-5):
        fit = att._lime_fit(x.to(dev), base.to(dev), mask.to(dev), S, 13, 16, interpretable_model=LM.SkLearnLasso(alpha=alpha))
        assert all(np.array_equal(a, b) for a, b in zip(fit["z"], z))
        assert np.all(np.abs(fit["w"] - w64) <= 1e-6 * w64)
        for b in range(B):
            y, w = fit["y"][:, b], fit["w"][:, b]
            # the engine's fit is the host fit of its own logits and weights, bit for bit, and optimal
            assert np.array_equal(refit(LM.SkLearnLasso(alpha=alpha), z[b], y, w), fit["coef"][b]), (alpha, b)
            c, icpt, _, _ = LM.lasso_fit(z[b], y, w, alpha)
            assert R.kkt_violation(z[b], y.astype(np.float64), w.astype(np.float64), alpha, c, icpt) * alpha <= 1e-9
            # against the same fit of the oracle's logits: the Lasso is piecewise linear in y, with slope ||M||_inf on an active set
            c_ref = LM.lasso_fit(z[b], y_oracle[b].astype(np.float32), w, alpha)[0]
            Minf = max([np.abs(R.active_set_map(z[b], w, cc)).sum(1).max(initial=0.0) for cc in (c, c_ref)])
            tol = TOL_LOGIT[precision] * max(1.0, np.abs(y_oracle[b]).max())
            err = np.abs(fit["coef"][b] - c_ref).max()
            bound = Minf * tol + 2 * U32 * np.abs(c_ref).max() + 1e-12
            print(f"Lime [{precision}] alpha {alpha} clip {b}: {np.count_nonzero(c_ref)} of {Ks[b]} active, max |coef - oracle fit| "
                  f"{err:.3e} (bound {bound:.3e}), logit spread {np.ptp(y_oracle[b]):.3e}")
            assert err <= bound
    attr = att.lime(x.to(dev), baselines=base.to(dev), feature_mask=mask.to(dev), n_samples=S, seed=13, internal_batch_size=16)
    fit = att._lime_fit(x.to(dev), base.to(dev), mask.to(dev), S, 13, 16)
    want = torch.stack([torch.from_numpy(fit["coef"][b])[index[b].long()] for b in range(B)])
    assert torch.equal(attr.cpu(), want)
    one = att.lime(x[:1].to(dev), baselines=base.to(dev), feature_mask=mask[:1].to(dev), n_samples=S, seed=13, return_input_shape=False)
    assert one.shape == (1, 6) and torch.equal(one.cpu()[0], torch.from_numpy(fit["coef"][0]))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_feature_permutation_against_the_oracle(gpu_device, precision):
    dev = gpu_device
    att, model = setup(dev, precision)
    B, L, K = 3, 16000, 5
    x = syn.make_clips(B, L, seed=62)
    mask = segments(L, K) - 2                                            # ids -2 .. 2
    ours = att.feature_permutation(x.to(dev), feature_mask=mask.to(dev), seed=14)
    index, _ = AT.feature_indices(mask, B, L)
    perm = AT.feature_permutation_draws(14, K, B)
    rows = torch.from_numpy(R.permuted_rows(x.numpy(), index.numpy(), perm))
    fwd = R.model_forward(model)
    f0, fk = fwd(x).view(-1), fwd(rows).view(-1)
    want = R.feature_permutation(x, index, perm, f0=f0, fk=fk)
    fmax = max(f0.abs().max().item(), fk.abs().max().item())
    bound = 2 * TOL_LOGIT[precision] * max(1.0, fmax)
    err = (ours.cpu() - want).abs().max().item()
    print(f"FeaturePermutation [{precision}]: max |err| vs oracle {err:.3e} (bound {bound:.3e}), max |attr| {want.abs().max():.3e}")
    assert err <= bound
    # FeatureAblation's arithmetic, bit for bit, on the engine's own logits (the same 15-row chunk)
    xd = x.to(dev)
    pts = torch.from_numpy(R.permuted_rows(x.numpy(), index.numpy(), perm)).to(dev)
    e0 = att.eg.emb.forward(xd, want_hidden=False)[1].view(-1).cpu()
    ek = att.eg.emb.forward(pts, want_hidden=False)[1].view(-1).cpu()
    assert torch.equal(ours.cpu(), R.feature_permutation(x, index, perm, f0=e0, fk=ek))


def test_chunking_and_seeds(gpu_device):
    dev = gpu_device
    att, _ = setup(dev, "f32")
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=63).to(dev)
    base = noise(1, L, 10).to(dev)
    mask = segments(L, 5).to(dev)
    lime = [att.lime(x, baselines=base, feature_mask=mask, n_samples=12, seed=21, internal_batch_size=ibs) for ibs in (1, 7, None)]
    fp = [att.feature_permutation(x, feature_mask=mask, seed=22, internal_batch_size=ibs) for ibs in (1, 7, None)]
    for name, outs in (("Lime", lime), ("FeaturePermutation", fp)):
        for o in outs[1:]:
            print(f"{name}: max |diff| across internal batches {(o - outs[0]).abs().max().item():.3e}")
            assert torch.equal(o, outs[0]), name
    assert torch.equal(att.lime(x, baselines=base, feature_mask=mask, n_samples=12, seed=21), lime[0])
    assert not torch.equal(att.lime(x, baselines=base, feature_mask=mask, n_samples=12, seed=23), lime[0])
    assert torch.equal(att.feature_permutation(x, feature_mask=mask, seed=22), fp[0])
    for fn in (lambda: att.lime(x, feature_mask=mask, n_samples=6), lambda: att.feature_permutation(x, feature_mask=mask)):
        torch.manual_seed(0)
        a = fn()
        torch.manual_seed(0)
        assert torch.equal(a, fn())


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import FeaturePermutation, Lime
    from captum._utils.models.linear_model import SkLearnLinearRegression, SkLearnRidge
    dev = gpu_device
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(dev)
    eng = model.hip_attribution()
    B, L, S = 2, 16000, 20
    x = syn.make_clips(B, L, seed=64).to(dev)
    base = noise(B, L, 13).to(dev)
    mask = segments(L, 5).to(dev)
    torch.manual_seed(1)
    a = Lime(model).attribute(x, baselines=base, feature_mask=mask, n_samples=S, perturbations_per_eval=3)
    torch.manual_seed(1)
    assert a.shape == x.shape and torch.equal(a, eng.lime(x, baselines=base, feature_mask=mask, n_samples=S))
    torch.manual_seed(2)
    f = FeaturePermutation(model).attribute(x, feature_mask=mask, perturbations_per_eval=2)
    torch.manual_seed(2)
    assert f.shape == x.shape and torch.equal(f, eng.feature_permutation(x, feature_mask=mask))
    torch.manual_seed(3)
    c = Lime(model).attribute(x[:1], feature_mask=mask, n_samples=S, return_input_shape=False)
    assert c.shape == (1, 5) and torch.isfinite(c).all()

    # a user similarity_func restating the cosine kernel, called per row, against the device weights
    def cosine_kernel(original, perturbed, interpretable, **kwargs):
        assert original.shape == perturbed.shape == (1, L) and interpretable.shape == (1, 5) and kwargs["num_interp_features"] == 5
        d = 1 - torch.nn.CosineSimilarity(dim=0)(original.reshape(-1).double(), perturbed.reshape(-1).double())
        return float(torch.exp(-d * d / 2))
    dev_fit = eng._lime_fit(x, base, mask, S, 5)
    user_fit = eng._lime_fit(x, base, mask, S, 5, similarity_func=cosine_kernel)
    err = np.abs(dev_fit["w"] - user_fit["w"]) / user_fit["w"]
    print(f"user cosine similarity_func vs device weights: max rel err {err.max():.3e}")
    assert err.max() <= 1e-6 and np.array_equal(dev_fit["y"], user_fit["y"])
    # the other interpretable models run, and fit the engine's data as they fit it directly
    for m, solve in ((SkLearnLinearRegression(), lambda z, y, w: AT.weighted_linear_fit(z, y, w)[0]),
                     (SkLearnRidge(alpha=0.5), lambda z, y, w: LM.ridge_fit(z, y, w, 0.5)[0])):
        fit = eng._lime_fit(x, base, mask, S, 7, interpretable_model=m)
        for b in range(B):
            want = solve(fit["z"][b].astype(np.float32), fit["y"][:, b], fit["w"][:, b]).astype(np.float32)
            assert np.array_equal(fit["coef"][b], want), type(m).__name__
        torch.manual_seed(4)
        out = Lime(model, interpretable_model=m).attribute(x, baselines=base, feature_mask=mask, n_samples=S)
        assert out.shape == x.shape and torch.isfinite(out).all()
    # a user perturb_func returning the engine's own Bernoulli table gives the default result, bit for bit
    table = iter([row for zb in AT.lime_draws(6, [5, 5], S) for row in zb])

    def replay(inp, **kwargs):
        assert inp.shape == (1, L) and kwargs["num_interp_features"] == 5 and kwargs["baselines"].shape == (1, L)
        assert kwargs["feature_mask"].shape == (1, L)
        return torch.from_numpy(next(table)[None].astype(np.int64)).to(inp.device)
    want = eng.lime(x, baselines=base, feature_mask=mask, n_samples=S, seed=6)
    assert torch.equal(Lime(model, perturb_func=replay).attribute(x, baselines=base, feature_mask=mask, n_samples=S), want)


def test_integration(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import FeaturePermutation, Lime, NoiseTunnel
    dev = gpu_device
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(dev)
    eng = model.hip_attribution()
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=65).to(dev)
    mask = segments(L, 4).to(dev)
    for method in (Lime(model), FeaturePermutation(model)):
        kw = {"n_samples": 10} if isinstance(method, Lime) else {}
        for nt_type in ("smoothgrad", "vargrad"):
            out = NoiseTunnel(method).attribute(x, nt_type=nt_type, nt_samples=3, nt_samples_batch_size=2, stdevs=0.01,
                                                feature_mask=mask, **kw)
            assert out.shape == x.shape and torch.isfinite(out).all(), (type(method).__name__, nt_type)
    seg = (torch.arange(L, device=dev) // 1600)[None]
    for method, fn in (("lime", lambda w: eng.lime(w, feature_mask=seg)), ("feature_permutation",
                                                                          lambda w: eng.feature_permutation(w, feature_mask=seg))):
        torch.manual_seed(4)
        p, t, m = cs.explain_waves(model, x, method=method)
        torch.manual_seed(4)
        attr = fn(x)
        _, w_rel, w_irr = eng.time_mask(attr, x)
        _, _, probs = runtime.hip_embedder().forward(torch.cat([x, w_rel, w_irr], 0), want_hidden=False)
        assert torch.equal(p, probs[:2]) and torch.equal(t, probs[2:4]) and torch.equal(m, probs[4:]), method
        sc = cs.score_explanations(model, x, method=method, n_perturb_samples=2)
        assert all(v.shape == (B,) and torch.isfinite(v).all() for v in sc.values()), (method, sc)
    with pytest.raises(ValueError):
        cs.explain_waves(model, x[:1], method="feature_permutation")
    # a non-finite logit raises, and so does a kernel under which every weight of a clip underflows to zero
    bad = x.clone()
    bad[1, 100] = float("inf")
    with pytest.raises(FloatingPointError):
        eng.lime(bad, feature_mask=mask, n_samples=4, seed=1)
    with pytest.raises(FloatingPointError):
        eng.feature_permutation(bad, feature_mask=mask, seed=1)
    with pytest.raises(FloatingPointError, match="clip 0.*kernel_width=0.001"):
        eng.lime(x, feature_mask=segments(L, 16).to(dev), n_samples=4, seed=1,
                 similarity_func=AT.ExpKernelSimilarity("euclidean", 1e-3))
    a = eng.lime(x, feature_mask=mask, n_samples=4, seed=1)                # the engine is usable after the errors
    assert torch.isfinite(a).all()


def test_lime_on_the_base_shape_is_finite(gpu_device):
    cfg = syn.base_config()
    sd = syn.embedder_weights(cfg)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision="f32"))
    L = 64000
    x = syn.make_clips(1, L, seed=66).to(gpu_device)
    mask = (torch.arange(L, device=gpu_device) // 1600)[None]
    a = att.lime(x, feature_mask=mask, n_samples=16, seed=1)
    c = att.lime(x, feature_mask=mask, n_samples=16, seed=1, return_input_shape=False)
    print(f"Lime on the wav2vec2-base shape (4 s, 40 segments, 16 samples): {np.count_nonzero(c.cpu().numpy())} non-zero, "
          f"max |coef| {c.abs().max().item():.3e}")
    assert a.shape == (1, L) and torch.isfinite(a).all() and torch.equal(a[0, ::1600].cpu(), c[0].cpu())
