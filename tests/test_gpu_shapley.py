"""GPU: the Shapley attributions (ShapleyValueSampling, ShapleyValues, KernelShap) on csrc/attribution_shapley.hip and the HIP
forward, against the Captum-style restatement of tests/shapley_ref.py: the coalition rows, the accumulation and the scatter bit
for bit; ShapleyValues against the exact subset formula on the oracle's CPU forward; the efficiency property; KernelShap's fit on
the engine's own logits; chunking and seeds; the captum.attr front end and explain_waves."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import shapley_ref as R
from addvisor_hip import attribution as AT, runtime, synthetic as syn
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


def test_coalition_rows_equal_the_restatement(gpu_device):
    dev = gpu_device
    B, K = 3, 4
    for L in (1000, 1001):                                               # float4 and scalar forms
        x = syn.make_clips(B, L, seed=L)
        g = torch.Generator().manual_seed(L)
        idx_b = torch.randint(0, K, (B, L), generator=g, dtype=torch.int32)
        for bname, base in (("scalar", torch.full((1, L), 0.25)), ("[1,L]", noise(1, L, 1)), ("[B,L]", noise(B, L, 2))):
            for index in (idx_b, idx_b[:1].contiguous()):
                # rank mode: a table of permutations 2, 3, 4
                p0, P = 2, 3
                rank = AT.shapley_permutations(L, p0 + P, K)[p0:]
                ref = R.permutation_rows(x, base, index, np.argsort(rank, axis=1))
                # presence mode: S coalitions per clip, row s * B + b
                S = 6
                z = AT.kernel_shap_draws(L, [K] * B, S)
                table = np.zeros((S * B, K), np.uint8)
                for b in range(B):
                    table[b::B] = z[b]
                kref = torch.stack([R.kernel_shap_rows(x, base, index[0 if index.shape[0] == 1 else b], z[b], b)[s]
                                    for s in range(S) for b in range(B)])
                for view in ("aligned", "misaligned"):
                    put = (lambda t: t.to(dev)) if view == "aligned" else (lambda t: misaligned(t.to(dev)))
                    xd, bd, idd = put(x), put(base), put(index)
                    rk, pr = torch.from_numpy(rank).to(dev), torch.from_numpy(table).to(dev)
                    what = (L, bname, list(index.shape), view)
                    d = AT.coalition_desc(xd, bd, idd, K, rank=rk, p0=p0)
                    out = torch.full((P * K * B, L), float("nan"), device=dev)
                    AT.coalition_points(d, p0 * K * B, P * K * B, out)
                    assert torch.equal(out.cpu(), ref), what
                    tail = torch.full((B + 4, L), float("nan"), device=dev)  # a chunk running past the table copies x[g % B]
                    end = (p0 + P) * K * B
                    AT.coalition_points(d, end - 2, B + 4, tail)
                    want = torch.cat([ref[-2:], x[[(end + i) % B for i in range(B + 2)]]])
                    assert torch.equal(tail.cpu(), want), what + ("rank tail",)
                    d = AT.coalition_desc(xd, bd, idd, K, present=pr)
                    out = torch.full((S * B, L), float("nan"), device=dev)
                    AT.coalition_points(d, 0, S * B, out)
                    assert torch.equal(out.cpu(), kref), what + ("presence",)
                    AT.coalition_points(d, S * B - 1, B + 4, tail)
                    want = torch.cat([kref[-1:], x[[(S * B + i) % B for i in range(B + 3)]]])
                    assert torch.equal(tail.cpu(), want), what + ("presence tail",)


def test_accumulate_and_scatter_bit_identical_to_the_restatement(gpu_device):
    dev = gpu_device
    B = 3
    g = torch.Generator().manual_seed(5)
    for L, K, P, groups in ((1000, 5, 7, (4, 3)), (1001, 3, 25, (25,)), (1001, 4, 24, (5, 5, 5, 5, 4))):
        index = torch.randint(0, K, (B, L), generator=g, dtype=torch.int32)
        if K == 4:                                                       # ShapleyValues: all 4! permutations, streamed
            nxt = AT.exact_permutation_stream(K)
            ranks = [nxt(G) for G in groups]
        else:
            nxt = AT._permutation_stream(L)
            ranks = [nxt(G, K) for G in groups]
        rank = np.concatenate(ranks)
        fbase = torch.randn(B, generator=g)
        fk = fbase.repeat(P * K) + 0.1 * torch.randn(P * K * B, generator=g)
        ref = R.shapley(torch.zeros(B, L), 0.0, index, np.argsort(rank, axis=1), fbase=fbase, fk=fk)
        x = torch.zeros(B, L, device=dev)
        base = torch.zeros(1, L, device=dev)
        idd = index.to(dev)
        total = torch.zeros(B, L, device=dev)
        p0 = 0
        for G, rk in zip(groups, ranks):
            rkd = torch.from_numpy(rk).to(dev)
            d = AT.coalition_desc(x, base, idd, K, rank=rkd, p0=p0)
            AT.shapley_accumulate(d, fbase.to(dev), fk[p0 * K * B:(p0 + G) * K * B].to(dev), p0, G, total,
                                  float(P) if p0 + G == P else 0.0)
            p0 += G
        assert torch.equal(total.cpu(), ref), (L, K, P, (total.cpu() - ref).abs().max())
        if K == 4:
            assert torch.equal(ref, R.shapley(torch.zeros(B, L), 0.0, index, R.all_permutations(4), fbase=fbase, fk=fk))
    for index in (index, index[:1].contiguous()):                        # the KernelShap scatter
        coef = torch.randn(B, K, generator=g)
        attr = torch.full((B, L), float("nan"), device=dev)
        idd, pr = index.to(dev), torch.zeros(1, K, dtype=torch.uint8, device=dev)        # alive while the desc points into them
        AT.coalition_scatter(AT.coalition_desc(x, base, idd, K, present=pr), coef.to(dev), attr)
        assert torch.equal(attr.cpu(), coef.gather(1, index.long().expand(B, L))), list(index.shape)


def coalition_logits(model, x, base, K):
    """F over all 2^K coalitions of K equal segments (oracle CPU forward, float64): ``{frozenset: [B]}``."""
    B, L = x.shape
    seg = segments(L, K)[0]
    fwd = R.model_forward(model)
    subsets = [frozenset(c) for n in range(K + 1) for c in itertools.combinations(range(K), n)]
    rows = torch.cat([R.coalition_row(x, base, torch.isin(seg, torch.tensor(sorted(s), dtype=torch.long)).float()[None].expand(B, L))
                      for s in subsets])
    f = fwd(rows).double().view(len(subsets), B)
    return dict(zip(subsets, f))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_shapley_values_equal_the_exact_subset_formula(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    B, L, K = 2, 16000, 4
    x = syn.make_clips(B, L, seed=51)
    base = noise(1, L, 7)
    F = coalition_logits(model, x, base, K)
    phi = torch.zeros(B, K, dtype=torch.float64)
    for i in range(K):
        for s, fs in F.items():
            if i not in s:
                w = math.factorial(len(s)) * math.factorial(K - len(s) - 1) / math.factorial(K)
                phi[:, i] += w * (F[s | {i}] - fs)
    ours = att.shapley_values(x.to(gpu_device), baselines=base.to(gpu_device), feature_mask=segments(L, K).to(gpu_device))
    want = phi.gather(1, segments(L, K, B)).float()
    fmax = max(f.abs().max().item() for f in F.values())
    bound = 2 * TOL_LOGIT[precision] * max(1.0, fmax)                   # the K! weights of each phi_i sum to 1
    err = (ours.cpu() - want).abs().max().item()
    print(f"ShapleyValues K = 4 [{precision}]: max |err| {err:.3e} (bound {bound:.3e}), phi {phi.tolist()}")
    assert err <= bound


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_efficiency(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    B, L, K, P = 2, 16000, 10, 25
    x = syn.make_clips(B, L, seed=52).to(gpu_device)
    base = noise(B, L, 8).to(gpu_device)
    mask = segments(L, K).to(gpu_device)
    # internal batch B: every forward has B rows, so F(row p, K - 1) = F(x) and F(base) are the logits below, bit for bit
    a = att.shapley_value_sampling(x, baselines=base, feature_mask=mask, n_samples=P, seed=3, internal_batch_size=B)
    fx, fb = att.logits(x).double().cpu(), att.logits(base).double().cpu()
    phi = a[:, ::L // K].double().cpu()                                  # one sample per feature
    fmax = max(fx.abs().max().item(), fb.abs().max().item())
    # per feature: P fp32 diffs (each |d| <= 2 fmax, rounded once), summed from 0 (P - 1 roundings of partial sums <= 2 P fmax),
    # one division; over K features
    bound = K * (P * U32 * 2 * fmax + (P - 1) * U32 * 2 * fmax + U32 * phi.abs().max().item()) + 1e-12
    err = (phi.sum(1) - (fx - fb)).abs().max().item()
    print(f"ShapleyValueSampling efficiency [{precision}]: max |sum phi - (F(x) - F(base))| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # KernelShap: the end coalitions weigh 1e6 against S - 2 unit weights, so the fit nearly interpolates them: the pull of the
    # unit rows on an end point is at most about (S - 2) * max |residual| / 1e6, and a residual is at most the spread of y
    S = 64
    fit = att._kernel_shap_fit(x, base, mask, S, 4, None)
    y = fit["y"]
    for b in range(B):
        coef, icpt = fit["coef"][b], fit["intercept"][b]
        full, empty = y[0, b], y[1, b]                                   # F(all ones) = F(x), F(all zeros) = F(base)
        kb = 4 * S * np.ptp(y[:, b]) / 1e6 + 1e-12
        print(f"KernelShap [{precision}] clip {b}: |icpt - F(base)| {abs(icpt - empty):.3e}, "
              f"|icpt + sum coef - F(x)| {abs(icpt + coef.sum() - full):.3e} (bound {kb:.3e})")
        assert abs(icpt - empty) <= kb and abs(icpt + coef.sum() - full) <= kb


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_kernel_shap_equals_the_restatement_on_its_own_logits(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    B, L = 2, 16001
    x = syn.make_clips(B, L, seed=53).to(gpu_device)
    base = noise(1, L, 9).to(gpu_device)
    mask = torch.stack([segments(L, 6)[0] * 2 + 1, segments(L, 8)[0] + 3]).to(gpu_device)     # different features per clip
    fit = att._kernel_shap_fit(x, base, mask, 40, 11, 16)
    index, Ks = AT.kernel_shap_feature_indices(mask.cpu(), B, L)
    assert Ks == [6, 8] and all(np.array_equal(a, b) for a, b in zip(fit["z"], AT.kernel_shap_draws(11, Ks, 40)))
    ref, coefs, icpts = R.kernel_shap(x.cpu(), base.cpu(), index, fit["z"], y=fit["y"])
    for b in range(B):
        assert np.allclose(fit["coef"][b], coefs[b], rtol=0, atol=1e-12 * max(1.0, np.abs(coefs[b]).max())), b
    ours = att.kernel_shap(x, baselines=base, feature_mask=mask, n_samples=40, seed=11, internal_batch_size=16)
    err = (ours.cpu() - ref).abs().max().item()
    print(f"KernelShap [{precision}] vs restatement on the engine's logits: max |err| {err:.3e}")
    assert err <= 2 * U32 * ref.abs().max().item()                       # the fp32 cast of equal float64 coefficients
    one = att.kernel_shap(x[:1], baselines=base, feature_mask=mask[:1], n_samples=40, seed=11, return_input_shape=False)
    fit1 = att._kernel_shap_fit(x[:1], base, mask[:1], 40, 11, None)
    assert one.shape == (6,) and torch.equal(one.cpu(), torch.from_numpy(fit1["coef"][0].astype(np.float32)))


def test_chunking_and_seeds(gpu_device):
    att, model = setup(gpu_device, "f32")
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=54).to(gpu_device)
    base = noise(1, L, 10).to(gpu_device)
    mask = segments(L, 5).to(gpu_device)
    svs = [att.shapley_value_sampling(x, baselines=base, feature_mask=mask, n_samples=6, seed=21, internal_batch_size=ibs)
           for ibs in (B, 7, 5 * B, None)]
    ks = [att.kernel_shap(x, baselines=base, feature_mask=mask, n_samples=30, seed=22, internal_batch_size=ibs) for ibs in (B, 7, None)]
    sv = [att.shapley_values(x, baselines=base, feature_mask=mask[:, :L] // 2, internal_batch_size=ibs) for ibs in (3, None)]
    for name, outs in (("ShapleyValueSampling", svs), ("KernelShap", ks), ("ShapleyValues", sv)):
        for o in outs[1:]:
            print(f"{name}: max |diff| across internal batches {(o - outs[0]).abs().max().item():.3e}")
            assert torch.equal(o, outs[0]), name
    assert torch.equal(att.shapley_value_sampling(x, baselines=base, feature_mask=mask, n_samples=6, seed=21), svs[0])
    assert not torch.equal(att.shapley_value_sampling(x, baselines=base, feature_mask=mask, n_samples=6, seed=23), svs[0])
    assert torch.equal(att.kernel_shap(x, baselines=base, feature_mask=mask, n_samples=30, seed=22), ks[0])
    torch.manual_seed(0)
    a = att.shapley_value_sampling(x, feature_mask=mask, n_samples=4)
    torch.manual_seed(0)
    assert torch.equal(a, att.shapley_value_sampling(x, feature_mask=mask, n_samples=4))


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import KernelShap, ShapleyValueSampling, ShapleyValues
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    x = syn.make_clips(2, 16000, seed=55).to(gpu_device)
    base = noise(2, 16000, 11).to(gpu_device)
    mask = segments(16000, 4).to(gpu_device)
    torch.manual_seed(1)
    a = ShapleyValueSampling(model).attribute(x, baselines=base, feature_mask=mask, n_samples=5, perturbations_per_eval=3)
    torch.manual_seed(1)
    assert a.shape == x.shape and torch.equal(a, eng.shapley_value_sampling(x, baselines=base, feature_mask=mask, n_samples=5))
    v = ShapleyValues(model).attribute(x, baselines=base, feature_mask=mask)
    assert torch.equal(v, eng.shapley_values(x, baselines=base, feature_mask=mask))
    torch.manual_seed(2)
    k = KernelShap(model).attribute(x, feature_mask=mask, n_samples=20)
    torch.manual_seed(2)
    assert torch.equal(k, eng.kernel_shap(x, feature_mask=mask, n_samples=20))
    torch.manual_seed(3)
    c = KernelShap(model).attribute(x[:1], feature_mask=mask, n_samples=20, return_input_shape=False)
    assert c.shape == (4,) and torch.isfinite(c).all()
    with pytest.raises(ValueError):
        ShapleyValueSampling(model).attribute(x, feature_mask=mask - 1)
    # explain_waves over 1600-sample segments (10 features per second) -> time mask -> three classifier passes
    for method, fn in (("shapley_value_sampling", eng.shapley_value_sampling), ("kernel_shap", eng.kernel_shap)):
        seg = (torch.arange(16000, device=gpu_device) // 1600)[None]
        torch.manual_seed(4)
        p, t, m = cs.explain_waves(model, x, method=method)
        torch.manual_seed(4)
        attr = fn(x, feature_mask=seg)
        _, w_rel, w_irr = eng.time_mask(attr, x)
        _, _, probs = runtime.hip_embedder().forward(torch.cat([x, w_rel, w_irr], 0), want_hidden=False)
        assert torch.equal(p, probs[:2]) and torch.equal(t, probs[2:4]) and torch.equal(m, probs[4:]), method
