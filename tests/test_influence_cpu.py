"""CPU-only: the float64 restatement of the influence methods (tests/influence_ref.py) is pinned by facts that do not depend on
it -- the influence-function score is the derivative of the refitted test loss with respect to a training weight and predicts
leave-one-out retraining, TracIn is torch autograd's per-sample gradient dot product, the similarities are torch's -- and the
bars of tests/test_gpu_influence.py have teeth.  Also the engine's argument errors that need no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import influence_ref as IR

FLAVOURS, IDS = [False, True], ["post_ln", "pre_ln"]
TOL = 1e-4                                                                   # the f32 bar of the GPU tests, of max|ref|


def relerr(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("l2", IR.L2S)
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_influence_function_is_the_derivative_of_the_refitted_loss(stable, l2):
    """Upweighting training clip n by eps (objective + eps * loss_n) moves the minimiser by ``-eps H^-1 grad l_n``, so the test
    loss moves by ``-eps S[t, n]``: a central difference with eps = 1e-4 over real refits, relative to max|S|, bar 1e-4.
    Leave-one-out retraining is eps = -1/N: Pearson correlation of ``S / N`` with the true loss change >= 0.99.
    Measured: differences 3.8e-7 to 3.0e-6; correlations 0.9902 to 0.9992; Hessian condition numbers 7.6e2 to 6.9e5."""
    c = IR.case(stable)
    Xn, yn, Xt, yt, v = c["Xn"], c["yn"], c["Xt"], c["yt"], c["theta"][l2]
    N, eps = len(yn), 1e-4
    S = IR.influence_functions(Xn, yn, Xt, yt, v, l2)
    base = IR.losses(Xt, yt, v)
    fd, loo = np.zeros_like(S), np.zeros_like(S)
    for n in range(N):
        w = np.ones(N)
        w[n] = 1.0 + eps * N                                                 # (1/N) sum w_i loss_i = the objective + eps loss_n
        up = IR.losses(Xt, yt, IR.newton_fit(Xn, yn, l2, w))
        w[n] = 1.0 - eps * N
        fd[:, n] = (up - IR.losses(Xt, yt, IR.newton_fit(Xn, yn, l2, w))) / (2 * eps)
        w[n] = 0.0
        loo[:, n] = IR.losses(Xt, yt, IR.newton_fit(Xn, yn, l2, w)) - base
    err = np.abs(fd + S).max() / np.abs(S).max()
    r = np.corrcoef(loo.ravel(), (S / N).ravel())[0, 1]
    print(f"l2={l2}: finite difference vs -S: {err:.3e} of max|S| = {np.abs(S).max():.3e}; leave-one-out Pearson r = {r:.4f}; "
          f"cond(H) = {np.linalg.cond(IR.hessian(Xn, v, l2)):.3e}")
    assert err <= 1e-4
    assert r >= 0.99


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_theta_is_the_minimiser_and_checkpoints_are_gradient_descent(stable):
    c = IR.case(stable)
    Xn, yn = c["Xn"], c["yn"]
    for l2, v in c["theta"].items():
        grad = (IR.sigmoid(Xn @ v) - yn) @ Xn / len(yn) + IR.reg_vector(len(v), l2) * v
        assert np.abs(grad).max() <= 1e-12
    v = np.zeros(Xn.shape[1])
    for (vk, lr), want in zip(c["checkpoints"], IR.LRS):
        v = v - lr * ((IR.sigmoid(Xn @ v) - yn) @ Xn / len(yn) + IR.reg_vector(len(v), 0.1) * v)
        assert lr == want and (vk == v).all() and np.isfinite(vk).all()


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_tracin_is_autograds_per_sample_gradient_dot_product(stable):
    c = IR.case(stable)
    Xn, yn, Xt, yt, cps = c["Xn"], c["yn"], c["Xt"], c["yt"], c["checkpoints"]
    H = Xn.shape[1] - 1

    def grads(lin, X, y):
        out = []
        for x, t in zip(torch.from_numpy(X[:, :H]), torch.from_numpy(y)):
            with torch.enable_grad():                                        # other test modules switch autograd off at import
                loss = F.binary_cross_entropy_with_logits(lin(x[None]).view(1), t.view(1), reduction="sum")
                gw, gb = torch.autograd.grad(loss, [lin.weight, lin.bias])
            out.append(torch.cat([gw.view(-1), gb.view(-1)]))
        return torch.stack(out)

    S = torch.zeros(len(Xt), len(Xn), dtype=torch.float64)
    self_inf = torch.zeros(len(Xn), dtype=torch.float64)
    for v, lr in cps:
        lin = torch.nn.Linear(H, 1).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(v[:H])[None])
            lin.bias.copy_(torch.tensor([v[H]]))
        gn, gt = grads(lin, Xn, yn), grads(lin, Xt, yt)
        S += lr * (gt @ gn.T)
        self_inf += lr * (gn * gn).sum(1)
    assert relerr(IR.tracin(Xn, yn, Xt, yt, cps), S.numpy()) <= 1e-13
    assert relerr(IR.tracin_self(Xn, yn, cps), self_inf.numpy()) <= 1e-13


@pytest.mark.parametrize("pool", ["none", "mean"])
def test_similarities_are_torchs(pool):
    c = IR.case(False)
    for l in IR.LAYERS:
        X, Y = IR.layer_features(c["ht"][l], pool).copy(), IR.layer_features(c["hn"][l], pool).copy()
        Y[3] = 0.0                                                           # a zero row: cosine 0 (Captum's replace_nan), not NaN
        tx, ty = torch.from_numpy(X), torch.from_numpy(Y)
        cos = IR.cosine_similarity(X, Y)
        want = (F.normalize(tx, dim=1) @ F.normalize(ty, dim=1).T).numpy()
        assert (cos[:, 3] == 0).all() and np.isfinite(cos).all()
        assert np.abs(np.delete(cos - want, 3, 1)).max() <= 1e-14
        assert relerr(IR.euclidean_distance(X, Y), torch.cdist(tx, ty, compute_mode="donot_use_mm_for_euclid_dist").numpy()) <= 1e-13
    idx, val = IR.topk(np.array([[1.0, 3.0, 3.0, -2.0, 1.0]]), 3)
    assert idx.tolist() == [[1, 2, 0]] and val.tolist() == [[3.0, 3.0, 1.0]]            # ties to the lower index
    idx, _ = IR.topk(np.array([[1.0, 3.0, 3.0, -2.0, 1.0]]), 3, largest=False)
    assert idx.tolist() == [[3, 0, 4]]


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_bars_have_teeth(stable):
    """A restatement that drops the bias column, the last feature column or one checkpoint misses the f32 bar of the GPU tests
    (1e-4 of max|ref|)."""
    c = IR.case(stable)
    Xn, yn, Xt, yt, cps = c["Xn"], c["yn"], c["Xt"], c["yt"], c["checkpoints"]
    T = IR.tracin(Xn, yn, Xt, yt, cps)

    def zeroed(X, col):
        X = X.copy()
        X[:, col] = 0.0
        return X

    # the residuals keep the full logit; the dropped column is missing from the gradient product alone
    def tracin_without(col):
        S = np.zeros_like(T)
        for v, lr in cps:
            S += lr * ((IR.sigmoid(Xt @ v) - yt)[:, None] * zeroed(Xt, col)) @ ((IR.sigmoid(Xn @ v) - yn)[:, None] * zeroed(Xn, col)).T
        return S

    wrong = {"no bias column": tracin_without(-1), "no last feature": tracin_without(-2), "two checkpoints": IR.tracin(Xn, yn, Xt, yt, cps[:2])}
    for l2 in IR.L2S:
        v = c["theta"][l2]
        S = IR.influence_functions(Xn, yn, Xt, yt, v, l2)
        for col, name in ((-1, "no bias column"), (-2, "no last feature")):
            keep = np.delete(np.arange(Xn.shape[1]), col % Xn.shape[1])
            gn = (IR.sigmoid(Xn @ v) - yn)[:, None] * Xn[:, keep]
            gt = (IR.sigmoid(Xt @ v) - yt)[:, None] * Xt[:, keep]
            e = relerr(gt @ np.linalg.solve(IR.hessian(Xn, v, l2)[np.ix_(keep, keep)], gn.T), S)
            print(f"influence functions, l2={l2}, {name}: {e:.3e}")
            assert e > TOL
    for name, S in wrong.items():
        print(f"TracIn, {name}: {relerr(S, T):.3e}")
        assert relerr(S, T) > TOL
    hn, ht = IR.layer_features(c["hn"][4], "mean"), IR.layer_features(c["ht"][4], "mean")
    for ref, fn in ((IR.cosine_similarity(ht, hn), IR.cosine_similarity), (IR.euclidean_distance(ht, hn), IR.euclidean_distance)):
        assert relerr(fn(ht[:, :-1], hn[:, :-1]), ref) > TOL


def test_argument_errors_without_a_device():
    from addvisor_hip import influence as INF
    with pytest.raises(TypeError):
        INF.HipInfluenceIndex(object())
    for cls, args in ((INF.HipSimilarityInfluence, (object(), 4)), (INF.HipTracInCPFast, (object(), [])), (INF.HipLogisticInfluence, (object(), 1.0))):
        with pytest.raises(TypeError):
            cls(*args)
    for bad in (torch.zeros(3), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3)):      # CPU tensors never reach a kernel
        for fn in (INF.moment, INF.sqdist, INF.sumsq, lambda t: INF.topk(t, 1)):
            with pytest.raises(ValueError):
                fn(bad)
    with pytest.raises(ValueError):
        INF.residual(torch.zeros(2, 3), torch.zeros(2))
    with pytest.raises(ValueError):
        INF._check_k(300, 1000)
    with pytest.raises(ValueError):
        INF._check_k(5, 4)
    assert INF._check_k(None, 4) is None and INF._check_k(4, 4) == 4
    from captum.influence import SimilarityInfluence, TracInCPFast, cosine_similarity, euclidean_distance
    with pytest.raises(TypeError):
        SimilarityInfluence(object(), ["hidden_states.4"], torch.zeros(2, 8))
    with pytest.raises(TypeError):
        TracInCPFast(object(), None, (torch.zeros(2, 8), torch.zeros(2)), [])
    assert cosine_similarity.__name__ == "cosine_similarity" and euclidean_distance.__name__ == "euclidean_distance"
