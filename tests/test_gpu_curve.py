"""GPU: the perturbation curves (deletion / insertion AUC, AOPC in MoRF / LeRF / random order) on csrc/attribution_curve.hip and
the HIP forward, against the numpy / float64 restatement of tests/curve_ref.py: the four kernels on their own (scores and curve
rows bit for bit, ranks exactly, the fold within 1e-6), the engine end to end with the oracle's CPU forward inside the logit
parity of tests/test_gpu_ablation.py, chunking and repeat determinism, the mask domain against tests/spectral_attr_ref.py, and
one wav2vec2-base run at 4 s.  Parity is unpinned: the metric is restated from the cited papers (no Captum class exists).

Measured on one MI355X (2026-10-19, this change on parent 79b9bbb).  Scores: bit-equal to the fp32 replay in every case, within
3.3e-4 of the bound n 2^-23 sum|a| of the float64 sum.  Ranks: exactly the stable double argsort for every K and score kind.
Curve rows: bit-equal, the MoRF / LeRF complement bit for bit.  Fold: probability curve <= 7.0e-8, auc <= 4.6e-8, aopc <= 8.1e-8
(bar 1e-6); logits of magnitude <= 13: auc <= 4.1e-7, aopc <= 3.6e-7 (bar 1e-6 max|y|).  End to end, tiny config, 2 clips x 1 s:
f32 logit curve <= 2.9e-6, probability curve <= 5.2e-7, auc <= 8.9e-7, aopc <= 2.2e-6 (bar 1e-4); f16 logit <= 5.9e-3, probability
<= 1.5e-3, auc <= 3.3e-3, aopc <= 3.8e-3 (bar 1e-2); ranks exact; every chunking and repeat bit-identical.  Mask domain: f32
7.8e-7 of max|ref| (bar 1e-4), f16 1.7e-3 (bar 3e-2).  wav2vec2-base, 2 clips x 4 s: step 0 / step S equal logits(x) to the bit;
deletion AUC on the probability MoRF 0.362 / 0.404, LeRF 0.568 / 0.492.  tools/bench_curve.py (wav2vec2-base shape, fp32-class,
16 clips x 4 s): curve_summary over 40 segments, S = 20, 672 rows: 130.0 ms, 0.981 of the plain forward over the same six
128-row chunks; per-sample deletion (K = 64 000), 336 rows: 68.9 ms, 0.925, the score + rank launches 4.13 ms = 6.0 % of the call
(K^2 = 4.1e9 key comparisons per clip).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ablation_ref as AR
import curve_ref as R
import spectral_attr_ref as SR
from addvisor_hip import attribution as AT, spectral_attribution as SA, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.spectral_attribution import HipSpectralAttribution

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}          # tests/test_gpu_ablation.py: the perturbation methods' logit parity
TOL_MASK = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}   # tests/test_gpu_spectral_attr.py: (max rel err, cosine) of its methods

_CACHE, _REF = {}, {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def ref_of(key, fn):
    """A reference computed once and shared by the tests (and precisions) that need it."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def numpy_forward(model, rows_per_call=16):
    fwd = AR.model_forward(model, rows_per_call)
    return lambda rows: fwd(torch.from_numpy(np.ascontiguousarray(rows))).numpy()


def offset_by_one_float(shape, dev):
    """An uninitialised fp32 tensor whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), device=dev)
    v = buf[1:].view(shape)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------------------- scores
def score_indices(n, B, rng):
    """name -> (index [1 | B, n] or None, K): the identity, contiguous 96-sample segments with a short last one, and shuffled
    per-clip indices with 300 features (two workgroups of 256 features, the second one partial) and with 257."""
    out = {"identity": (None, n), "segments": ((np.arange(n) // 96)[None].astype(np.int32), -(-n // 96))}
    for K in (300, 257):
        idx = np.stack([rng.permutation(np.concatenate([np.arange(K), rng.integers(0, K, n - K)])) for _ in range(B)])
        out[f"shuffled{K}"] = (idx.astype(np.int32), K)
    return out


@pytest.mark.parametrize("n", [1000, 1001])
def test_scores_bit_for_bit_against_the_replay(gpu_device, n):
    B = 3
    rng = np.random.default_rng(n)
    a = rng.standard_normal((B, n)).astype(np.float32)
    a[0, 3], a[1, 7] = -0.0, 0.0
    ad = torch.from_numpy(a).to(gpu_device)
    worst = 0.0
    for name, (index, K) in score_indices(n, B, rng).items():
        idx_d = None if index is None else torch.from_numpy(index).to(gpu_device)
        for use_abs in (False, True):
            for mean in (False, True):
                got = AT.feature_scores(ad, idx_d, K, use_abs, mean).cpu().numpy()
                want = R.scores32_replay(a, index, K, use_abs, mean)
                assert got.shape == (B, K) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, use_abs, mean)
                ref = R.scores64(a, index, K, use_abs, mean)
                err, bound = np.abs(got - ref), n * 2.0 ** -23 * np.abs(a).sum(1, keepdims=True)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (name, use_abs, mean)
    print(f"scores n={n}: bit-equal to the fp32 replay; worst |err| / (n 2^-23 sum|a|) vs float64 = {worst:.3e}")
    gap = torch.from_numpy(np.array([[0, 0, 2, 2] * (n // 4) + [0] * (n % 4)], np.int32)).to(gpu_device)      # feature 1 has no sample
    s = AT.feature_scores(ad, gap, 3).cpu()
    assert torch.isneginf(s[:, 1]).all() and torch.isfinite(s[:, [0, 2]]).all()


# ------------------------------------------------------------------------------------------------------------------------ rank
# One path serves every K: a workgroup ranks 1024 features (256 threads x 4) against LDS tiles of 2048 keys.  1023 / 1024 / 1025
# straddle the workgroup edge, 2047 / 2048 / 2049 the key-tile edge; 4097 and 16001 take several of both with partial last ones.
RANK_K = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16001]


def rank_scores(kind, B, K, rng):
    s = rng.standard_normal((B, K)).astype(np.float32)
    if kind == "ties":
        s = np.round(s * 2).clip(-4, 3).astype(np.float32)              # 8 values
    elif kind == "all_equal":
        s = np.full((B, K), -1.5, np.float32)
    elif kind == "zeros_infs":
        pick = rng.integers(0, 6, (B, K))
        for v, val in enumerate((0.0, -0.0, np.inf, -np.inf)):
            s[pick == v] = val
    return s


@pytest.mark.parametrize("K", RANK_K)
def test_rank_equals_the_stable_argsort(gpu_device, K):
    B = 3
    rng = np.random.default_rng(K)
    for kind in ("random", "ties", "all_equal", "zeros_infs"):
        s = rank_scores(kind, B, K, rng)
        sd = torch.from_numpy(s).to(gpu_device)
        for descending in (True, False):
            got = AT.feature_rank(sd, descending).cpu().numpy()
            key = -s.astype(np.float64) if descending else s.astype(np.float64)
            want = np.argsort(np.argsort(key, axis=1, kind="stable"), axis=1, kind="stable")
            assert got.dtype == np.int32 and np.array_equal(got, want), (K, kind, descending)
            assert all(np.array_equal(np.sort(r), np.arange(K)) for r in got), (K, kind, descending)


# ---------------------------------------------------------------------------------------------------------------------- points
@pytest.mark.parametrize("n", [1000, 1001])
def test_points_bit_equal_to_the_reference_rows(gpu_device, n):
    dev = gpu_device
    B, K = 3, 11
    rng = np.random.default_rng(n + 1)
    x, base = rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, n)).astype(np.float32)
    index = rng.integers(0, K, (B, n)).astype(np.int32)
    score = rng.standard_normal((B, K)).astype(np.float32)               # tie-free
    morf, lerf = R.rank_argsort(score, True), R.rank_argsort(score, False)
    counts = np.array([0, 1, 4, 9, K], np.int32)
    S1 = len(counts)
    total = S1 * B
    plans = [[(0, total)], [(0, 7), (7, 7), (14, 7)], [(2, 5), (13, 6)]]   # a step split across chunks; 6 / 4 padding rows at the end
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(counts).to(dev)
    for base_rows in (1, B):
        for index_rows in (1, B):
            bs, ix = base[:base_rows], index[:index_rows]
            bd, ixd = torch.from_numpy(bs).to(dev), torch.from_numpy(ix).to(dev)
            for mode in (0, 1):
                want = R.rows(x, bs, ix, morf, counts, mode, n_rows=total + 6)
                assert np.array_equal(want[total:], x[[g % B for g in range(total, total + 6)]])
                d = AT.curve_desc(xd, bd, ixd, torch.from_numpy(morf).to(dev), cd, mode)
                for view in ("aligned", "offset"):
                    for plan in plans:
                        for row0, rows in plan:
                            out = torch.full((rows, n), float("nan"), device=dev) if view == "aligned" else offset_by_one_float((rows, n), dev)
                            AT.curve_points(d, row0, rows, out)
                            assert np.array_equal(out.cpu().numpy().view(np.uint32), want[row0:row0 + rows].view(np.uint32)), \
                                (n, base_rows, index_rows, mode, view, row0, rows)
                # deletion in MoRF order at c == insertion in LeRF order at K - c, bit for bit
                back = torch.empty((total, n), device=dev)
                AT.curve_points(AT.curve_desc(xd, bd, ixd, torch.from_numpy(lerf).to(dev), torch.from_numpy(K - counts[::-1].copy()).to(dev),
                                              1 - mode), 0, total, back)
                mine = torch.empty((total, n), device=dev)
                AT.curve_points(d, 0, total, mine)
                assert torch.equal(mine.view(S1, B, n), back.view(S1, B, n).flip(0)), (n, base_rows, index_rows, mode)
    # an out-of-range feature index gives NaN in exactly those samples, every step; the padding rows copy x
    bad = index.copy()
    bad[1, 5], bad[2, n - 1], bad[0, 0] = K, -1, 2 ** 30
    d = AT.curve_desc(xd, torch.from_numpy(base).to(dev), torch.from_numpy(bad).to(dev), torch.from_numpy(morf).to(dev), cd, 0)
    out = torch.empty((total + 2, n), device=dev)
    AT.curve_points(d, 0, total + 2, out)
    want = np.zeros((total + 2, n), bool)
    want[1:total:B, 5], want[2:total:B, n - 1], want[0:total:B, 0] = True, True, True
    assert np.array_equal(np.isnan(out.cpu().numpy()), want)
    # the identity index (K == n)
    rank_n = R.rank_argsort(rng.standard_normal((B, n)), True)
    cn = np.array([0, n // 3, n], np.int32)
    d = AT.curve_desc(xd, torch.from_numpy(base[:1]).to(dev), None, torch.from_numpy(rank_n).to(dev), torch.from_numpy(cn).to(dev), 1)
    out = torch.empty((3 * B, n), device=dev)
    AT.curve_points(d, 0, 3 * B, out)
    assert np.array_equal(out.cpu().numpy(), R.rows(x, base[:1], None, rank_n, cn, 1))


# ------------------------------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("S1", [2, 3, 21])
def test_fold_against_float64(gpu_device, S1):
    B, K = 5, 97
    rng = np.random.default_rng(S1)
    inner = [np.sort(rng.choice(np.arange(lo, hi), S1 - 2, replace=False)) for lo, hi in ((1, K), (4, K - 1))]    # uneven steps
    for cts in (np.concatenate([[0], inner[0], [K]]), np.concatenate([[3], inner[1], [K - 1]])):       # the second: f_0 > 0, f_last < 1
        cts = cts.astype(np.int32)
        n = len(cts)
        fk = (4 * rng.standard_normal(n * B)).astype(np.float32)
        fkd, cd = torch.from_numpy(fk).to(gpu_device), torch.from_numpy(cts).to(gpu_device)
        for prob in (True, False):
            for ref_last in (False, True):
                curve, auc, aopc = (t.cpu().double().numpy() for t in AT.curve_fold(fkd, cd, B, K, prob, ref_last))
                y, a, o = R.fold(fk, cts, B, K, prob, ref_last)
                scale = 1.0 if prob else float(np.abs(y).max())
                errs = [float(np.abs(curve - y).max()), float(np.abs(auc - a).max()), float(np.abs(aopc - o).max())]
                print(f"fold S1={n} prob={prob} ref_last={ref_last}: |err| curve {errs[0]:.2e} auc {errs[1]:.2e} aopc {errs[2]:.2e} (bar {1e-6 * scale:.2e})")
                assert max(errs[:2]) <= 1e-6 * scale and errs[2] <= 2e-6 * scale        # aopc: a difference carries two values
    bad = torch.tensor([0, 5, 5] + list(range(6, 6 + S1 - 3)), dtype=torch.int32)[:S1] if S1 > 2 else torch.tensor([4, 4], dtype=torch.int32)
    _, auc, aopc = AT.curve_fold(torch.zeros(S1 * B, device=gpu_device), bad.to(gpu_device), B, K, True, False)
    assert torch.isnan(auc).all() and torch.isnan(aopc).all()            # counts that do not increase strictly


# ------------------------------------------------------------------------------------------------------------------ end to end
EB, EL = 2, 16000
ORDERS = ("morf", "lerf", "random")
SEED = 1234


def e2e_clips():
    return syn.make_clips(EB, EL, seed=46)


def e2e_reference(model, x, attr, index, K, steps, mode, order):
    """The oracle's logits of the reference rows, folded both ways: {prob: (curve, fractions, auc, aopc, rank)}."""
    rank = AT.shapley_permutations(SEED, EB, K) if order == "random" else None
    fk = {}

    def forward(rows):
        fk["fk"] = numpy_forward(model)(rows)
        return fk["fk"]
    out = {True: R.perturbation_curve(forward, x, attr, mode, order, index, K, steps, 0.0, True, rank=rank)}
    curve, auc, aopc = R.fold(fk["fk"], R.counts_from_steps(steps, K), EB, K, False, mode == "insertion")
    out[False] = (curve, out[True][1], auc, aopc, out[True][4])
    return out


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("source", ["seeded", "input_x_gradient"])
@pytest.mark.parametrize("features", ["segments", "samples"])
def test_end_to_end_against_the_oracle_forward(gpu_device, features, source, precision):
    att, model = setup(gpu_device, precision)
    x = e2e_clips()
    xd = x.to(gpu_device)
    if source == "seeded":
        attr = torch.randn(EB, EL, generator=torch.Generator().manual_seed(9))
    else:
        attr = att.input_x_gradient(xd).cpu()                            # the engine's own map: both sides rank identical bits
    if features == "segments":
        mask, index, K, steps = (torch.arange(EL) // 1600)[None], (np.arange(EL) // 1600)[None], 10, None
    else:
        mask, index, K, steps = None, None, EL, 8
    tol = TOL_LOGIT[precision]
    f0 = att.logits(xd).cpu().double().numpy()
    worst = {"logit": 0.0, "prob": 0.0, "auc": 0.0, "aopc": 0.0}
    for mode in ("deletion", "insertion"):
        for order in ORDERS:
            key = (features, mode, order) + (("seeded",) if source == "seeded" else (source, precision))
            ref = ref_of(key, lambda: e2e_reference(model, x.numpy(), attr.numpy(), index, K, steps, mode, order))
            for output in ("logit", "prob"):
                got = att.perturbation_curve(xd, attr.to(gpu_device), mode=mode, order=order, feature_mask=mask, steps=steps, output=output,
                                             seed=SEED)
                curve, frac, auc, aopc, rank = ref[output == "prob"]
                assert got.curve.shape == (EB, len(frac)) and got.rank.dtype == torch.int32
                assert np.array_equal(got.rank.cpu().numpy(), rank), (mode, order)
                assert np.array_equal(got.fractions.cpu().numpy(), frac)
                e_curve = float(np.abs(got.curve.cpu().double().numpy() - curve).max())
                e_auc = float(np.abs(got.auc.cpu().double().numpy() - auc).max())
                e_aopc = float(np.abs(got.aopc.cpu().double().numpy() - aopc).max())
                worst[output] = max(worst[output], e_curve)
                worst["auc"], worst["aopc"] = max(worst["auc"], e_auc), max(worst["aopc"], e_aopc)
                assert e_curve <= tol and e_auc <= tol, (mode, order, output, e_curve, e_auc)
                assert e_aopc <= 2 * tol, (mode, order, output, e_aopc)   # a difference carries two outputs
                if output == "logit":                                    # the reference step is the clip itself: no separate F(x)
                    step = 0 if mode == "deletion" else -1
                    assert float(np.abs(got.curve[:, step].cpu().double().numpy() - f0).max()) <= tol
    print(f"end to end {features} {source} [{precision}]: max |err| logit curve {worst['logit']:.3e}, prob curve {worst['prob']:.3e}, "
          f"auc {worst['auc']:.3e}, aopc {worst['aopc']:.3e} (bar {tol:.0e})")


def test_chunking_and_repeat_are_bit_identical(gpu_device):
    att, _ = setup(gpu_device, "f32")
    xd = e2e_clips().to(gpu_device)
    attr = torch.randn(EB, EL, generator=torch.Generator().manual_seed(9)).to(gpu_device)
    mask = (torch.arange(EL) // 1600)[None]
    base = (0.05 * torch.randn(EB, EL, generator=torch.Generator().manual_seed(3))).to(gpu_device)
    for kw in (dict(mode="deletion", order="morf", feature_mask=mask, baselines=base), dict(mode="insertion", order="lerf", steps=8),
               dict(mode="deletion", order="random", seed=5, feature_mask=mask, output="logit", use_abs=True, pool="mean")):
        first = att.perturbation_curve(xd, attr, internal_batch_size=EB, **kw)
        for ibs in (5, 128, EB):
            again = att.perturbation_curve(xd, attr, internal_batch_size=ibs, **kw)
            for a, b in zip(first, again):
                assert torch.equal(a, b), (kw, ibs)
    s1, s2 = att.curve_summary(xd, attr, feature_mask=mask), att.curve_summary(xd, attr, feature_mask=mask, internal_batch_size=5)
    assert sorted(s1) == ["comprehensiveness", "deletion_auc", "insertion_auc", "sufficiency"]
    dele = att.perturbation_curve(xd, attr, feature_mask=mask)
    ins = att.perturbation_curve(xd, attr, mode="insertion", feature_mask=mask)
    for k, want in (("deletion_auc", dele.auc), ("insertion_auc", ins.auc), ("comprehensiveness", dele.aopc), ("sufficiency", ins.aopc)):
        assert torch.equal(s1[k], want) and torch.equal(s2[k], want) and s1[k].shape == (EB,), k
    with pytest.raises(ValueError):
        att.perturbation_curve(xd, torch.full_like(attr, float("nan")), feature_mask=mask)


def test_front_end(gpu_device):
    import captum_saliency as cs

    class Wave:
        def hip_attribution(self):
            return setup(gpu_device, "f32")[0]
    att = Wave().hip_attribution()
    xd = e2e_clips().to(gpu_device)
    attr = att.input_x_gradient(xd)
    out = cs.evaluate_explanation(Wave(), xd, attr, segment=1600, steps=5)
    want = att.curve_summary(xd, attr, feature_mask=(torch.arange(EL) // 1600)[None], steps=5)
    assert all(torch.equal(out[k], want[k]) for k in want)


# ----------------------------------------------------------------------------------------------------------------- mask domain
MB, ML, CROP = 2, 16000, (512, 48)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_mask_domain_against_the_restatement(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    clips = syn.make_clips(MB, ML, seed=12)
    eng = ref_of(("mask engine", precision), lambda: HipSpectralAttribution(att, clips.to(gpu_device), "linear"))
    mm = ref_of("mask model", lambda: SR.MaskModel(clips, model, "linear"))
    Fm, Tm = CROP
    g = torch.Generator().manual_seed(5)
    m = 0.25 + 0.75 * torch.rand(MB, Fm, Tm, generator=g)
    attr = torch.randn(MB, Fm, Tm, generator=g)
    ids = SA.tf_feature_mask(Fm, Tm, 64, 16)
    index, K = AT.shapley_feature_indices(ids.view(1, -1), MB, Fm * Tm)
    assert K == 24
    fwd = mm.flat_forward(Fm, Tm)
    forward = lambda rows: fwd(torch.from_numpy(np.ascontiguousarray(rows))).numpy()   # noqa: E731
    tol, cmin = TOL_MASK[precision]
    for mode, order in (("deletion", "morf"), ("insertion", "lerf")):
        ref = ref_of(("mask", mode, order), lambda: R.perturbation_curve(forward, m.view(MB, -1).numpy(), attr.view(MB, -1).numpy(), mode,
                                                                         order, index.numpy(), K, steps=6, base=0.5, prob=True))
        got = eng.perturbation_curve(m.to(gpu_device), attr.to(gpu_device), mode=mode, order=order, feature_mask=ids, steps=6, baselines=0.5)
        assert np.array_equal(got.rank.cpu().numpy(), ref[4])
        ours, want = got.curve.cpu().double(), torch.from_numpy(ref[0])
        err = ((ours - want).abs().max() / want.abs().max()).item()
        cos = F.cosine_similarity(ours.flatten(), want.flatten(), dim=0).item()
        e_auc = float(np.abs(got.auc.cpu().double().numpy() - ref[2]).max() / np.abs(ref[2]).max())
        print(f"mask curve {mode} {order} [{precision}]: max rel err {err:.3e}, cosine {cos:.8f}, auc rel err {e_auc:.3e}")
        assert err < tol and cos > cmin and e_auc < tol, (mode, order, err, cos, e_auc)
    s = eng.curve_summary(m.to(gpu_device), attr.to(gpu_device), feature_mask=ids, steps=6, baselines=0.5)
    assert sorted(s) == ["comprehensiveness", "deletion_auc", "insertion_auc", "sufficiency"]
    assert all(v.shape == (MB,) and bool(torch.isfinite(v).all()) for v in s.values())
    with pytest.raises(NotImplementedError):
        eng.kernel_shap(m.to(gpu_device))


# ---------------------------------------------------------------------------------------------------------------- wav2vec2-base
BASE_SEED = 51


def test_wav2vec2_base_at_4s(gpu_device):
    """2 clips x 4 s, K = 40 segments of 100 ms, S = 20: 42 rows, one forward chunk.  The inequality below was verified on the
    CPU oracle for this seed first (clips of seed 51, the oracle's own FeatureAblation map: deletion AUC on the probability MoRF
    0.362 / 0.404 against LeRF 0.568 / 0.492, on the logit -0.589 / -0.396 against 0.281 / -0.032)."""
    att, _ = setup(gpu_device, "f32", "base")
    B, L = 2, 64000
    x = syn.make_clips(B, L, seed=BASE_SEED).to(gpu_device)
    mask = (torch.arange(L) // 1600)[None]
    attr = att.feature_ablation(x, feature_mask=mask)
    f0 = att.logits(x)
    morf = att.perturbation_curve(x, attr, feature_mask=mask, steps=20, output="logit")
    lerf = att.perturbation_curve(x, attr, order="lerf", feature_mask=mask, steps=20, output="logit")
    ins = att.perturbation_curve(x, attr, mode="insertion", feature_mask=mask, steps=20, output="logit")
    assert morf.curve.shape == (B, 21) and all(bool(torch.isfinite(t).all()) for r in (morf, lerf, ins) for t in r)
    tol = TOL_LOGIT["f32"]
    e0 = max((morf.curve[:, 0] - f0).abs().max().item(), (lerf.curve[:, 0] - f0).abs().max().item(), (ins.curve[:, -1] - f0).abs().max().item())
    print(f"base 4 s: F(x) {f0.tolist()}, step-0 / step-S vs F(x) max |err| {e0:.3e}; deletion auc (logit) MoRF {morf.auc.tolist()} "
          f"LeRF {lerf.auc.tolist()}")
    assert e0 <= tol
    pm = att.perturbation_curve(x, attr, feature_mask=mask, steps=20)
    pl = att.perturbation_curve(x, attr, order="lerf", feature_mask=mask, steps=20)
    print(f"base 4 s: deletion auc (prob) MoRF {pm.auc.tolist()} LeRF {pl.auc.tolist()}")
    assert bool((pm.auc <= pl.auc).all()) and bool((morf.auc <= lerf.auc).all())
