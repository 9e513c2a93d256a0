"""GPU: training-data influence on the HIP chain (csrc/influence.hip, addvisor_hip/influence.py, captum/influence).  Kernel
level: the moment, squared-distance, sum-of-squares and top-k kernels are exact on integer-valued data (every partial sum is an
integer below 2^24) at every tail, stride and alignment, bit-identical from run to run, and within 8 x numpy's own fp32 error on
real-valued data; the elementwise kernels equal float64 numpy rounded once.  Engine level: similarity, TracInCPFast and influence
functions against the float64 restatement of tests/influence_ref.py driven by the oracle, the index's behaviour, the
captum.influence front end and the range contract."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import concept_ref as CR
import influence_ref as IR
from addvisor_hip import _lib, influence as INF, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999)}                                             # the bar of the layer attributions (test_gpu_layer_attr.py)
# f16 chain: scores vs the restatement, relative to max|ref|.  Measured over both LayerNorm flavours, both pools, layers 0 and 4,
# both metrics, TracIn and its self-influence, on the MI355X: at most 8.983e-4 (post-LN, euclidean, layer 4, pool="mean"; pre-LN at
# most 6.884e-4; TracIn 7.640e-4 / 6.262e-4).  The bound is twice that.
F16_SCORE_TOL = 1.7966e-3
FLAVOURS, IDS = [False, True], ["post_ln", "pre_ln"]


def ints(rows, cols, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def layouts(x, dev):
    """The same matrix as a contiguous tensor, with row stride F + 4 (16-byte aligned rows), with row stride F + 1 (4-byte
    loads), and starting one float into a buffer (``buf[:, 1:]``: a base pointer that is not 16-byte aligned)."""
    M, Fx = x.shape
    out = {"contiguous": x.to(dev)}
    for name, pad in (("ld=F+4", 4), ("ld=F+1", 1)):
        buf = torch.full((M, Fx + pad), 7.0, device=dev)                     # the padding is never read: 7s would show
        buf[:, :Fx] = x.to(dev)
        out[name] = buf[:, :Fx]
    buf = torch.full((M, Fx + 1), 7.0, device=dev)
    buf[:, 1:] = x.to(dev)
    out["base+1"] = buf[:, 1:]
    assert out["base+1"].data_ptr() % 16 == 4 and out["ld=F+4"].stride(0) == Fx + 4
    return out


def twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b), "not bit-identical from run to run"
    return a


# ------------------------------------------------------------------------------------------------ kernels, exact
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "w"])
@pytest.mark.parametrize("N,Fx", [(1, 1), (3, 5), (70, 65), (130, 129), (1100, 193)])
def test_moment_is_exact_on_integers(gpu_device, N, Fx, weighted):
    """(1100, 193): three slabs of the rows (512 + 512 + 76) and ten blocks; (130, 129): a block of one column."""
    x = ints(N, Fx, 1)
    w = ints(1, N, 2, 0, 4).view(-1) if weighted else None
    xl = x.long().numpy()
    ref = torch.from_numpy((xl * (w.long().numpy()[:, None] if weighted else 1)).T @ xl).double()
    wd = None if w is None else w.to(gpu_device)
    for name, X in layouts(x, gpu_device).items():
        Hm = twice(lambda: INF.moment(X, wd))
        assert Hm.dtype == torch.float64 and torch.equal(Hm.cpu(), ref), name
        assert torch.equal(Hm, Hm.T.contiguous()), name                      # mirrored entries: the same bits


@pytest.mark.parametrize("M,N,Fx", [(1, 1, 1), (5, 3, 1000), (3, 4, 1029), (70, 65, 130), (33, 33, 4099)])
def test_sqdist_is_exact_on_integers(gpu_device, M, N, Fx):
    x, y = ints(M, Fx, 3), ints(N, Fx, 4)
    ref = torch.from_numpy(((x.long().numpy()[:, None] - y.long().numpy()[None]) ** 2).sum(-1)).double()
    for lx, X in layouts(x, gpu_device).items():
        for ly, Y in layouts(y, gpu_device).items():
            D = twice(lambda: INF.sqdist(X, Y))
            assert D.dtype == torch.float64 and torch.equal(D.cpu(), ref), (lx, ly)
        D = twice(lambda: INF.sqdist(X))                                     # X is Y
        assert bool((D.diagonal() == 0).all()) and torch.equal(D, D.T.contiguous()), lx


@pytest.mark.parametrize("M,Fx", [(1, 1), (2, 7), (33, 4099), (70, 3136)])
def test_sumsq_is_exact_on_integers(gpu_device, M, Fx):
    x = ints(M, Fx, 5)
    ref = torch.from_numpy((x.long().numpy() ** 2).sum(1)).double()
    for name, X in layouts(x, gpu_device).items():
        s = twice(lambda: INF.sumsq(X))
        assert s.dtype == torch.float64 and torch.equal(s.cpu(), ref), name


@pytest.mark.parametrize("M,N,C", [(1, 1, 1), (3, 70, 3), (6, 1000, 5)])
def test_elementwise_kernels_round_once(gpu_device, M, N, C):
    """residual, cosine, root, scale and self_scale against float64 numpy rounded once to fp32: equal to the bit, or within
    1 ulp where the sigmoid (the device's exp) is involved.  A zero norm gives 0."""
    rng = np.random.default_rng(M * 1000 + N)
    dev = gpu_device
    Z = 6.0 * rng.standard_normal((N, C))
    Z.flat[0], Z.flat[-1] = 800.0, -800.0                                    # no overflow on either side
    y = (rng.random(N) < 0.5).astype(np.float32)
    r = twice(lambda: INF.residual(torch.from_numpy(Z).to(dev), torch.from_numpy(y).to(dev))).cpu().numpy()
    want = np.where(y[None] == 1, -IR.sigmoid(-Z.T), IR.sigmoid(Z.T)).astype(np.float32)   # sigma(z) - 1 == -sigma(-z), no cancellation
    assert r.shape == (C, N) and np.isfinite(r).all()
    ulps = np.abs(r.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"residual ({N},{C}): max {ulps.max():.2f} ulp, {np.count_nonzero(r != want)} of {r.size} entries differ")
    assert ulps.max() <= 1.0

    G = rng.standard_normal((M, N))
    a, b = rng.random(M) + 0.1, rng.random(N) + 0.1
    a[0], b[-1] = 0.0, 0.0
    Gd = torch.from_numpy(G).to(dev)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = G / (np.sqrt(a)[:, None] * np.sqrt(b)[None])
    want[(a == 0)[:, None] | (b == 0)[None]] = 0.0
    cos = twice(lambda: INF.cosine(Gd, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    assert torch.equal(cos.cpu(), torch.from_numpy(want.astype(np.float32)))
    assert bool((cos[0] == 0).all()) and bool((cos[:, -1] == 0).all())
    wide = torch.full((M, N + 3), 7.0, device=dev)                           # ldo > N: the padding is not written
    INF.root(Gd.abs(), out=wide[:, :N])
    assert torch.equal(wide[:, :N].cpu(), torch.from_numpy(np.sqrt(np.abs(G)).astype(np.float32))) and bool((wide[:, N:] == 7).all())

    lr = rng.random(C) + 0.01
    rt, rn = rng.standard_normal((C, M)).astype(np.float32), rng.standard_normal((C, N)).astype(np.float32)
    s = np.zeros((M, N))
    for c in range(C):
        s = s + (lr[c] * rt[c].astype(np.float64))[:, None] * rn[c].astype(np.float64)[None]
    lrd, rtd, rnd = torch.from_numpy(lr).to(dev), torch.from_numpy(rt).to(dev), torch.from_numpy(rn).to(dev)
    out = twice(lambda: INF.scale(Gd, rtd, rnd, lrd))
    assert torch.equal(out.cpu(), torch.from_numpy((G * s).astype(np.float32)))
    ss = rng.random(N) * 50
    d = np.zeros(N)
    for c in range(C):
        d = d + (lr[c] * rn[c].astype(np.float64)) * rn[c].astype(np.float64)
    out = twice(lambda: INF.self_scale(torch.from_numpy(ss).to(dev), rnd, lrd))
    assert torch.equal(out.cpu(), torch.from_numpy((ss * d).astype(np.float32)))


@pytest.mark.parametrize("largest", [1, 0])
@pytest.mark.parametrize("M,N,k", [(1, 1, 1), (3, 7, 7), (2, 1000, 5), (5, 4099, 64), (2, 70000, 256)])
def test_topk_is_stable_argsort(gpu_device, M, N, k, largest):
    """Integer data in -3..3: heavy ties, which go to the lower index.  (5, 4099, 64): three chunks; (2, 70000, 256): 35
    chunks whose 8960 kept keys are five chunks more -- three passes.  Row stride > N."""
    s = ints(M, N, 6)
    s[0, 0] = -0.0                                                           # -0.0 ties with +0.0
    ri, rv = IR.topk(s.numpy(), k, bool(largest))
    for name in ("contiguous", "ld=F+4", "base+1"):
        S = layouts(s, gpu_device)[name]
        idx, val = INF.topk(S, k, bool(largest))
        idx2, val2 = INF.topk(S, k, bool(largest))
        assert torch.equal(idx, idx2) and torch.equal(val, val2)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), ri), name
        assert np.array_equal(val.cpu().numpy(), rv), name


def test_topk_real_values(gpu_device):
    """Distinct real values of both signs, denormals and infinities excluded: the order of the orderable bits."""
    g = torch.Generator().manual_seed(7)
    s = torch.randn(3, 5000, generator=g) * torch.tensor([1e-20, 1.0, 1e20])[:, None]
    for largest in (True, False):
        idx, val = INF.topk(s.to(gpu_device), 100, largest)
        ri, rv = IR.topk(s.numpy(), 100, largest)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv)


# ------------------------------------------------------------------------------------------------ kernels, real-valued
def term_error(got, ref, scale):
    return float((np.abs(np.asarray(got, np.float64) - ref) / scale).max())


@pytest.mark.parametrize("N,Fx", [(3136, 70), (4099, 33)])
def test_moment_real_valued_error(gpu_device, N, Fx):
    """Per entry, relative to ``sum_i |w x x|``, against float64: within 8 x the error of numpy's own fp32
    ``(X32 * w32[:, None]).T @ X32`` (computed here; the factor is for the different summation order)."""
    X32 = CR.gram_real_inputs(N, Fx)
    w32 = np.random.default_rng(8).random(N).astype(np.float32)
    X64, w64 = X32.astype(np.float64), w32.astype(np.float64)
    X = torch.from_numpy(X32).to(gpu_device)
    for name, w in (("ones", None), ("w", w32)):
        wr = np.ones(N) if w is None else w64
        ref, scale = (X64 * wr[:, None]).T @ X64, (np.abs(X64) * wr[:, None]).T @ np.abs(X64)
        own = X32.T @ X32 if w is None else (X32 * w32[:, None]).T @ X32
        bound = 8.0 * term_error(own, ref, scale)
        Hm = INF.moment(X, None if w is None else torch.from_numpy(w32).to(gpu_device))
        err = term_error(Hm.cpu().numpy(), ref, scale)
        print(f"moment ({N},{Fx}) {name}: error {err:.3e} of sum|wxx|; numpy fp32 {bound / 8:.3e}; bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        assert torch.equal(Hm, Hm.T.contiguous())


def test_sqdist_real_valued_error(gpu_device):
    """(33, 33, 4099): per entry, relative to ``sum_f (x - y)^2`` (every term is positive), against float64: within 8 x the
    error of numpy's own fp32 ``((X32[:, None] - Y32[None]) ** 2).sum(-1)``.  With X is Y: zero diagonal, bitwise symmetric."""
    M, N, Fx = 33, 33, 4099
    X32, Y32 = CR.gram_real_inputs(M, Fx), CR.gram_real_inputs(N, Fx, seed=6)
    ref = ((X32.astype(np.float64)[:, None] - Y32.astype(np.float64)[None]) ** 2).sum(-1)
    bound = 8.0 * term_error(((X32[:, None] - Y32[None]) ** 2).sum(-1, dtype=np.float32), ref, ref)
    X, Y = torch.from_numpy(X32).to(gpu_device), torch.from_numpy(Y32).to(gpu_device)
    err = term_error(INF.sqdist(X, Y).cpu().numpy(), ref, ref)
    print(f"sqdist ({M},{N},{Fx}): error {err:.3e} of sum (x-y)^2; numpy fp32 {bound / 8:.3e}; bound {bound:.3e}")
    assert err <= bound
    D = INF.sqdist(X)
    assert bool((D.diagonal() == 0).all()) and torch.equal(D, D.T.contiguous())
    near = X.clone()
    near[:, 5] += 1e-3                                                       # near-duplicates: a + b - 2G would cancel to noise
    d = INF.sqdist(X, near).diagonal().cpu().numpy()
    want = (near[:, 5] - X[:, 5]).double().cpu().numpy() ** 2
    assert np.abs(d - want).max() <= 1e-6 * want.max()


# ------------------------------------------------------------------------------------------------ engine
_ATT, _IDX = {}, {}


def engine(dev, precision, stable=False):
    key = (stable, precision)
    if key not in _ATT:
        sd, cfg, coef, icpt = IR.case_model(stable)
        _ATT[key] = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))
    return _ATT[key]


def index(dev, precision, stable, pool="none"):
    """The case's training set, embedded once per (flavour, precision, pool) and shared; tests must not add to it."""
    key = (stable, precision, pool)
    if key not in _IDX:
        _IDX[key] = INF.HipInfluenceIndex(engine(dev, precision, stable), IR.LAYERS, pool=pool).add(IR.train_clips().to(dev), IR.train_labels())
    return _IDX[key]


def relerr(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / (np.abs(ref).max() + 1e-300))


def cosine(a, ref):
    return F.cosine_similarity(torch.as_tensor(np.asarray(a, np.float64)).flatten(), torch.as_tensor(ref).flatten(), dim=0).item()


def checkpoints_of(c):
    return [(v[:-1], v[-1], lr) for v, lr in c["checkpoints"]]


def similarity_cases(dev, precision, stable, pool):
    """``(name, device scores [B, N], reference)`` for both metrics at both layers."""
    c, ix = IR.case(stable), index(dev, precision, stable, pool)
    x = IR.test_clips().to(dev)
    for l in IR.LAYERS:
        ht, hn = IR.layer_features(c["ht"][l], pool), IR.layer_features(c["hn"][l], pool)
        for metric, fn in (("cosine", IR.cosine_similarity), ("euclidean", IR.euclidean_distance)):
            S = INF.HipSimilarityInfluence(ix, l, metric).influence(x, top_k=None)
            yield f"{metric} layer {l} pool={pool}", S.cpu().numpy(), fn(ht, hn)


def tracin_cases(dev, precision, stable):
    c, ix = IR.case(stable), index(dev, precision, stable)
    tr = INF.HipTracInCPFast(ix, checkpoints_of(c))
    S = tr.influence(IR.test_clips().to(dev), IR.test_labels())
    yield "TracIn", S.cpu().numpy(), IR.tracin(c["Xn"], c["yn"], c["Xt"], c["yt"], c["checkpoints"])
    yield "TracIn self-influence", tr.self_influence().cpu().numpy(), IR.tracin_self(c["Xn"], c["yn"], c["checkpoints"])


@pytest.mark.parametrize("pool", ["none", "mean"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_similarity_parity_f32(gpu_device, stable, pool):
    tol, cmin = TOL["f32"]
    for name, S, ref in similarity_cases(gpu_device, "f32", stable, pool):
        e, cs = relerr(S, ref), cosine(S, ref)
        print(f"[f32] {name}: err {e:.3e} cos {cs:.8f}")
        assert S.shape == ref.shape == (IR.N_TEST, IR.N_TRAIN) and S.dtype == np.float32
        assert e < tol and cs > cmin, name


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_tracin_parity_f32(gpu_device, stable):
    tol, cmin = TOL["f32"]
    for name, S, ref in tracin_cases(gpu_device, "f32", stable):
        e, cs = relerr(S, ref), cosine(S, ref)
        print(f"[f32] {name}: err {e:.3e} cos {cs:.8f}")
        assert S.shape == ref.shape and e < tol and cs > cmin, name


def own_features(ix, dev):
    """The device's own pooled features of the case, downloaded: ``(Xn, Xt)`` float64, augmented."""
    return ix.phi.cpu().double().numpy(), ix.embed(IR.test_clips().to(dev))[0].cpu().double().numpy()


def own_feature_check(ix, dev, c, l2, tag):
    """Influence functions against the reference evaluated on the device's own features, at the reference's theta.  The bar is
    10 x the error that a numpy-fp32 Hessian followed by the same float64 solve shows on those features (the margin is for the
    summation order)."""
    Xn, Xt = own_features(ix, dev)
    v = c["theta"][l2]
    ref = IR.influence_functions(Xn, c["yn"], Xt, c["yt"], v, l2)
    p = IR.sigmoid(Xn @ v)
    X32, w32 = Xn.astype(np.float32), (p * (1 - p)).astype(np.float32)
    H32 = ((X32 * w32[:, None]).T @ X32).astype(np.float64) / len(Xn) + np.diag(IR.reg_vector(Xn.shape[1], l2))
    bar = 10.0 * relerr(IR.influence_functions(Xn, c["yn"], Xt, c["yt"], v, l2, hess=H32), ref)
    S = INF.HipLogisticInfluence(ix, l2, coef=v[:-1], intercept=v[-1]).influence(IR.test_clips().to(dev), IR.test_labels())
    e = relerr(S.cpu().numpy(), ref)
    print(f"[{tag}] influence functions l2={l2}, own features: err {e:.3e}; numpy-fp32 Hessian {bar / 10:.3e}; bar {bar:.3e}; "
          f"cond(H) {np.linalg.cond(IR.hessian(Xn, v, l2)):.3e}")
    return e, bar


@pytest.mark.parametrize("l2", IR.L2S)
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_influence_functions_parity_f32(gpu_device, stable, l2):
    c, ix = IR.case(stable), index(gpu_device, "f32", stable)
    e, bar = own_feature_check(ix, gpu_device, c, l2, "f32")
    assert e <= bar
    # end to end against the oracle-driven reference: theta is fitted on the device's features.  The bar is the largest move of
    # the reference's own scores when its features move by up to 1e-4 of max|feature| (the project's hidden-state bar; uniform,
    # five seeds) and theta is refitted.
    Xn, Xt, yn, yt = c["Xn"], c["Xt"], c["yn"], c["yt"]
    ref = IR.influence_functions(Xn, yn, Xt, yt, c["theta"][l2], l2)
    amp = 1e-4 * np.abs(Xn[:, :-1]).max()
    moves = []
    for seed in range(5):
        rng = np.random.default_rng(seed)
        Pn, Pt = Xn.copy(), Xt.copy()
        Pn[:, :-1] += amp * rng.uniform(-1, 1, Pn[:, :-1].shape)
        Pt[:, :-1] += amp * rng.uniform(-1, 1, Pt[:, :-1].shape)
        moves.append(relerr(IR.influence_functions(Pn, yn, Pt, yt, IR.newton_fit(Pn, yn, l2), l2), ref))
    li = INF.HipLogisticInfluence(ix, l2)
    coef, icpt, its = li.fit()
    S = li.influence(IR.test_clips().to(gpu_device), IR.test_labels())
    e2 = relerr(S.cpu().numpy(), ref)
    print(f"[f32] influence functions l2={l2}, oracle reference: err {e2:.3e}; bar {max(moves):.3e} (moves {[f'{m:.2e}' for m in moves]}); "
          f"fit: {its} iterations, theta err {np.abs(np.append(coef, icpt) - c['theta'][l2]).max():.3e}")
    assert e2 <= max(moves)


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_topk_at_engine_level(gpu_device, stable):
    """No tie exemptions: the value returned for index idx[m, j] is the reference's value there, and the returned values are the
    reference's sorted top-k values, both within the f32 tolerance of max|ref| (sorting is 1-Lipschitz in the max norm)."""
    tol = TOL["f32"][0]
    c, ix = IR.case(stable), index(gpu_device, "f32", stable, "mean")
    x, N = IR.test_clips().to(gpu_device), IR.N_TRAIN
    tr = INF.HipTracInCPFast(ix, checkpoints_of(c))
    rt = IR.tracin(c["Xn"], c["yn"], c["Xt"], c["yt"], c["checkpoints"])
    rs = IR.cosine_similarity(IR.layer_features(c["ht"][4], "mean"), IR.layer_features(c["hn"][4], "mean"))
    for k in (1, 5, N):
        for largest in (True, False):
            runs = (("TracIn", tr.influence(x, IR.test_labels(), k=k, proponents=largest), rt),
                    ("cosine", INF.HipSimilarityInfluence(ix, 4, "cosine", "max" if largest else "min").influence(x, top_k=k), rs))
            for name, (idx, val), ref in runs:
                assert idx.dtype == torch.int64 and tuple(idx.shape) == tuple(val.shape) == (IR.N_TEST, k)
                i, v = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
                assert all(len(set(row)) == k for row in i.tolist())
                bar = tol * np.abs(ref).max()
                assert np.abs(np.take_along_axis(ref, i, 1) - v).max() <= bar, (name, k, largest)
                assert np.abs(IR.topk(ref, k, largest)[1] - v).max() <= bar, (name, k, largest)


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_parity_f16(gpu_device, stable):
    """The fp16-operand chain, scores only: similarity (both pools), TracIn and its self-influence within F16_SCORE_TOL of
    max|ref|; influence functions against the reference on the chain's own features (the f32 test's first check)."""
    worst = 0.0
    cases = [t for pool in ("none", "mean") for t in similarity_cases(gpu_device, "f16", stable, pool)] + list(tracin_cases(gpu_device, "f16", stable))
    for name, S, ref in cases:
        e = relerr(S, ref)
        worst = max(worst, e)
        print(f"[f16] {name}: err {e:.3e}")
    print(f"[f16] largest error {worst:.3e}")
    c, ix = IR.case(stable), index(gpu_device, "f16", stable)
    for l2 in IR.L2S:
        e, bar = own_feature_check(ix, gpu_device, c, l2, "f16")
        assert e <= bar
    assert worst < F16_SCORE_TOL


# ------------------------------------------------------------------------------------------------ behaviour
def test_index_chunking_and_two_adds(gpu_device):
    att = engine(gpu_device, "f32")
    x, y = IR.train_clips()[:12].to(gpu_device), IR.train_labels()[:12]
    a = INF.HipInfluenceIndex(att, IR.LAYERS, internal_batch_size=16).add(x, y)
    b = INF.HipInfluenceIndex(att, IR.LAYERS, internal_batch_size=5).add(x, y)          # 5 + 5 + 2
    two = INF.HipInfluenceIndex(att, IR.LAYERS).add(x[:7], y[:7]).add(x[7:], y[7:])
    assert a.n == b.n == two.n == 12 and a.phi.stride(0) % 4 == 0 and tuple(a.phi.shape) == (12, 65)
    assert bool((a.phi[:, -1] == 1).all())                                   # the bias column
    for other in (b, two):
        # the chain is batch-invariant (tests/test_gpu_layer_attr.py asserts equal bits over its chunk sizes): so is the index
        assert torch.equal(a.phi, other.phi) and torch.equal(a.labels, other.labels)
        for l in IR.LAYERS:
            assert torch.equal(a.activations(l), other.activations(l))
    assert tuple(a.activations(4).shape) == (12, 49 * 64)
    with pytest.raises(ValueError, match="labels"):
        INF.HipInfluenceIndex(att).add(x).labels
    with pytest.raises(ValueError, match="0 or 1"):
        INF.HipInfluenceIndex(att).add(x, np.arange(12))


def test_index_save_load_budget_and_frames(gpu_device, tmp_path):
    att = engine(gpu_device, "f32")
    x, y = IR.train_clips()[:6].to(gpu_device), IR.train_labels()[:6]
    a = INF.HipInfluenceIndex(att, [4]).add(x, y)
    path = str(tmp_path / "index.npz")
    a.save(path)
    with np.load(path, allow_pickle=False) as z:                             # no pickle inside
        assert sorted(z.files) == ["labels", "layer_4", "phi", "settings"]
    b = INF.HipInfluenceIndex(att, [4]).load(path)
    assert torch.equal(a.phi, b.phi) and torch.equal(a.activations(4), b.activations(4)) and torch.equal(a.labels, b.labels)
    assert b.phi.stride(0) % 4 == 0
    sa = INF.HipSimilarityInfluence(a, 4).influence(x[:2], top_k=3)
    sb = INF.HipSimilarityInfluence(b, 4).influence(x[:2], top_k=3)
    assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
    assert sa[0][:, 0].tolist() == [0, 1]                                    # a training clip's nearest neighbour is itself
    for other in (INF.HipInfluenceIndex(att, [4], pool="mean"), INF.HipInfluenceIndex(att, [0]),
                  INF.HipInfluenceIndex(engine(gpu_device, "f16"), [4])):
        with pytest.raises(ValueError, match="other settings"):
            other.load(path)
    with pytest.raises(MemoryError, match="memory_budget"):
        INF.HipInfluenceIndex(att, IR.LAYERS, memory_budget=6 * 49 * 64 * 4).add(x, y)
    short = syn.make_clips(4, 8000, seed=1).to(gpu_device)
    with pytest.raises(ValueError, match="frame count"):
        INF.HipInfluenceIndex(att, [4]).add(x, y).add(short, y[:4])
    m = INF.HipInfluenceIndex(att, [4], pool="mean").add(x, y).add(short, y[:4])          # lengths may differ
    assert tuple(m.activations(4).shape) == (10, 64)


def test_hessian_must_be_positive_definite(gpu_device):
    ix = index(gpu_device, "f32", False)                                     # N = 40 < H + 1 = 65
    with pytest.raises(ValueError, match="damping"):
        INF.HipLogisticInfluence(ix, 0.0, damping=0.0).influence(IR.test_clips().to(gpu_device), IR.test_labels())
    S = INF.HipLogisticInfluence(ix, 0.0, damping=1e-3).influence(IR.test_clips().to(gpu_device), IR.test_labels())
    assert bool(torch.isfinite(S).all())


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_fit_reproduces_the_reference_theta(gpu_device, stable):
    """Given the same features (the device's own, downloaded), ``fit()`` and the reference's float64 Newton fit agree to 1e-8
    of max|theta|."""
    ix = index(gpu_device, "f32", stable)
    Xn = ix.phi.cpu().double().numpy()
    for l2 in IR.L2S:
        coef, icpt, its = INF.HipLogisticInfluence(ix, l2).fit()
        ref = IR.newton_fit(Xn, IR.train_labels(), l2)
        err = np.abs(np.append(coef, icpt) - ref).max() / np.abs(ref).max()
        print(f"fit l2={l2}: {its} iterations, err {err:.3e} of max|theta| = {np.abs(ref).max():.3e}")
        assert err <= 1e-8 and its < 50


def test_range_contract(gpu_device):
    """A saturating activation (one FFN bias entry of 1e5, as tests/test_gpu_training.py) still raises SplitRangeError through
    add(), and the next valid call succeeds."""
    sd, cfg, coef, icpt = IR.case_model(False)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["encoder.layers.0.feed_forward.intermediate_dense.bias"][3] = 1e5
    bad = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision="f32"))
    x, y = IR.train_clips()[:4].to(gpu_device), IR.train_labels()[:4]
    with pytest.raises(_lib.SplitRangeError):
        INF.HipInfluenceIndex(bad, [4]).add(x, y)
    torch.cuda.synchronize()
    _lib.lib().advh_split_overflow(1)
    ix = INF.HipInfluenceIndex(engine(gpu_device, "f32"), [4]).add(x, y)
    assert bool(torch.isfinite(ix.phi).all())


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.influence import SimilarityInfluence, TracInCPFast, cosine_similarity, euclidean_distance
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    train, y = IR.train_clips()[:12].to(gpu_device), IR.train_labels()[:12]
    x, yx = IR.test_clips()[:3].to(gpu_device), IR.test_labels()[:3]
    front = SimilarityInfluence(model, ["hidden_states.4", 0], [train[:5], train[5:]], similarity_metric=euclidean_distance,
                                similarity_direction="min")
    out = front.influence(x, top_k=3)
    ix = INF.HipInfluenceIndex(eng, [4, 0]).add(train)
    assert sorted(out, key=str) == [0, "hidden_states.4"]
    for name, l in (("hidden_states.4", 4), (0, 0)):
        idx, val = INF.HipSimilarityInfluence(ix, l, "euclidean", "min").influence(x, top_k=3)
        assert torch.equal(out[name][0], idx) and torch.equal(out[name][1], val)
        assert bool((val[:, 1:] >= val[:, :-1]).all())                       # nearest first
    cos = SimilarityInfluence(model, 4, train, similarity_metric=cosine_similarity).influence(train[:2])[4]
    assert cos[0].view(-1).tolist() == [0, 1] and tuple(cos[1].shape) == (2, 1)
    H = eng.eg.cfg.hidden_size
    g = torch.Generator().manual_seed(3)
    cps = [(0.05 * torch.randn(H, generator=g), 0.1 * c, 0.5 / (c + 1)) for c in range(2)]
    tf = TracInCPFast(model, None, [(train[:5], y[:5]), (train[5:], y[5:])], cps)
    direct = INF.HipTracInCPFast(INF.HipInfluenceIndex(eng).add(train, y), cps)
    assert torch.equal(tf.influence((x, yx)), direct.influence(x, yx))
    pi, pv = tf.influence((x, yx), k=4, proponents=False)
    di, dv = direct.influence(x, yx, k=4, proponents=False)
    assert torch.equal(pi, di) and torch.equal(pv, dv) and torch.equal(tf.self_influence(), direct.self_influence())
    with pytest.raises(NotImplementedError):
        TracInCPFast(model, None, (train, y), cps, checkpoints_load_func=lambda m, p: 0.1)
    with pytest.raises(NotImplementedError):
        TracInCPFast(model, None, (train, y), cps, loss_fn=torch.nn.BCEWithLogitsLoss())
    with pytest.raises(NotImplementedError):
        SimilarityInfluence(model, 4, train, similarity_metric=lambda a, b: a @ b.T)
    with pytest.raises(NotImplementedError):
        SimilarityInfluence(model, 4, train, activation_dir="acts")
    with pytest.raises(ValueError):
        SimilarityInfluence(model, ["hidden_states.10"], train)
