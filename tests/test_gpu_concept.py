"""GPU: TCAV on the HIP chain (csrc/concept.hip, addvisor_hip/concept.py, captum/concept).  Kernel level: the Gram, combine and
time-pool kernels are exact on integer-valued data (every partial sum is an integer below 2^24) at every tail, stride and
alignment, bit-identical from run to run, and within 8 x numpy's own fp32 error on real-valued data.  Engine level: CAVs,
scores, sign counts, accuracies and magnitudes against the float64 restatement of tests/concept_ref.py, the closed form at the
last layer, chunking, sharing of activations, the per-frame map, the captum.concept front end and the range contract."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import concept_ref as CR
from addvisor_hip import _lib, concept as CO, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999)}                                             # the bar of the layer attributions (test_gpu_layer_attr.py)
# f16 chain: scores vs the restatement, relative to max|ref|.  Measured over both LayerNorm flavours, both pools, layers 0 and 4,
# both sets, on the MI355X: at most 1.658e-2 (pre-LN, pool="mean", R2/R1, layer 4; every other case <= 8.9e-3).
# The bound is twice that.  The reference's scores leave at most one of the 8 inputs per (set, layer, concept) inside that band
# (post-LN: R2/R1 at layer 0 with 4.7e-3 of max|ref|, A/R1 at layer 0 with pool="mean" with 2.6e-2; the next is 3.46e-2).
F16_SCORE_TOL = 3.32e-2
FLAVOURS, IDS = [False, True], ["post_ln", "pre_ln"]


def ints(rows, cols, seed):
    return torch.randint(-3, 4, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


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
@pytest.mark.parametrize("M,N,Fx", [(1, 1, 1), (2, 2, 7), (5, 3, 1000), (8, 6, 3136), (3, 4, 1029), (70, 65, 130)])
def test_gram_cross_is_exact_on_integers(gpu_device, M, N, Fx):
    """(3, 4, 1029): two full slabs of 512 plus 5.  (70, 65, 130): more than one block along both M and N."""
    x, y = ints(M, Fx, 1), ints(N, Fx, 2)
    ref = torch.from_numpy(x.long().numpy() @ y.long().numpy().T)
    for lx, X in layouts(x, gpu_device).items():
        for ly, Y in layouts(y, gpu_device).items():
            G = twice(lambda: CO.gram(X, Y))
            assert G.dtype == torch.float64 and torch.equal(G.cpu().long(), ref) and torch.equal(G.cpu(), ref.double()), (lx, ly)


@pytest.mark.parametrize("M,Fx", [(1, 1), (2, 7), (33, 4099), (70, 3136), (130, 200)])
def test_gram_symmetric_is_exact_and_mirrored(gpu_device, M, Fx):
    x = ints(M, Fx, 3)
    ref = torch.from_numpy(x.long().numpy() @ x.long().numpy().T).double()
    for name, X in layouts(x, gpu_device).items():
        G = twice(lambda: CO.gram(X))
        assert torch.equal(G.cpu(), ref), name
        assert torch.equal(G, G.T.contiguous()), name                        # mirrored entries: the same bits
        assert torch.equal(CO.gram(X, X.clone()), G), name                   # the cross form of the same product


@pytest.mark.parametrize("C,N,Fx", [(1, 1, 1), (2, 5, 7), (3, 17, 1000), (2, 24, 3136), (9, 5, 260), (17, 3, 66)])
def test_combine_is_exact_on_integers(gpu_device, C, N, Fx):
    """C = 9 and 17: more than one group of eight coefficient rows."""
    a, x = ints(C, N, 4), ints(N, Fx, 5)
    ref = torch.from_numpy(a.long().numpy() @ x.long().numpy()).float()
    for name, X in layouts(x, gpu_device).items():
        W = twice(lambda: CO.combine(a.to(gpu_device), X))
        assert W.dtype == torch.float32 and torch.equal(W.cpu(), ref), name


def test_combine_is_one_fmaf_chain(gpu_device):
    """Real-valued: the fp32 chain ``acc = fma(a_i, x_i, acc)`` over ascending i, replayed on the host.  The product of two
    fp32 numbers is exact in float64, so ``float32(a * x + acc)`` computed in float64 is the fused result except for a double
    rounding (one case in about 2^29): at most two entries may differ, by one ulp; another summation order would move most."""
    g = torch.Generator().manual_seed(6)
    a, x = torch.randn(3, 24, generator=g), torch.randn(24, 1001, generator=g)
    W = twice(lambda: CO.combine(a.to(gpu_device), x.to(gpu_device))).cpu().numpy()
    acc = np.zeros((3, 1001), np.float32)
    for i in range(24):
        acc = (a[:, i].double().numpy()[:, None] * x[i].double().numpy()[None] + acc.astype(np.float64)).astype(np.float32)
    diff = np.abs(W.astype(np.float64) - acc)
    print(f"combine vs the host fmaf chain: {np.count_nonzero(diff)} of {diff.size} entries differ, max {diff.max():.3e}")
    assert np.count_nonzero(diff) <= 2 and diff.max() <= 2.0 ** -22 * np.abs(W).max()      # double rounding at most, never another order
    ref = a.double() @ x.double()
    assert (torch.from_numpy(W).double() - ref).abs().max() <= 24 * 2.0 ** -24 * (a.abs().double() @ x.abs().double()).max()


@pytest.mark.parametrize("H", [64, 65])
@pytest.mark.parametrize("T", [1, 49])
def test_time_pool(gpu_device, T, H):
    R = 3
    xi = torch.randint(-3, 4, (R, T, H), generator=torch.Generator().manual_seed(7)).float()
    s = twice(lambda: CO.time_pool(xi.to(gpu_device)))
    assert torch.equal(s.cpu(), xi.long().sum(1).float())                    # mode 0, integers: exact
    xr = torch.randn(R, T, H, generator=torch.Generator().manual_seed(8))
    acc = np.zeros((R, H), np.float32)
    for t in range(T):
        acc = acc + xr[:, t].numpy()                                         # fp32, t ascending
    assert torch.equal(twice(lambda: CO.time_pool(xr.to(gpu_device))).cpu(), torch.from_numpy(acc))
    mean = twice(lambda: CO.time_pool(xr.to(gpu_device), mean=True))
    assert torch.equal(mean.cpu(), torch.from_numpy(acc * np.float32(1.0 / T)))           # mode 1: the sum times float(1 / T)
    out = torch.empty(R, H, device=gpu_device)
    assert CO.time_pool(xr.to(gpu_device), mean=True, out=out) is out and torch.equal(out, mean)


# ------------------------------------------------------------------------------------------------ kernels, real-valued
@pytest.mark.parametrize("M,N,Fx", CR.GRAM_REAL_SHAPES)
def test_gram_real_valued_error(gpu_device, M, N, Fx):
    """Per entry, relative to ``sum_f |x y|``, against float64: within 8 x the error of numpy's own fp32 ``X32 @ X32.T`` at the
    same shape (computed here).  Measured on the MI355X: 4.39e-7 at (70, 70, 3136) and 3.23e-7 at (33, 33, 4099), against
    numpy's 3.10e-7 and 3.38e-7.  tests/test_concept_cpu.py shows that the bound has teeth."""
    X32 = CR.gram_real_inputs(M, Fx)
    X64 = X32.astype(np.float64)
    bound = CR.gram_bound(X32)
    X = torch.from_numpy(X32).to(gpu_device)
    for name, G in (("symmetric", CO.gram(X)), ("cross", CO.gram(X, X.clone()))):
        err = CR.gram_error(G.cpu().numpy(), X64, X64)
        print(f"gram ({M},{N},{Fx}) {name}: error {err:.3e} of sum|xy|; numpy fp32 {bound / 8:.3e}; bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


# ------------------------------------------------------------------------------------------------ engine
_ATT = {}


def engine(dev, precision, stable=False):
    key = (stable, precision)
    if key not in _ATT:
        sd, cfg, coef, icpt = CR.case_model(stable)
        _ATT[key] = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))
    return _ATT[key]


def concepts_on(dev):
    waves = CR.case_concepts()
    return {cid: CO.Concept(cid, f"c{cid}", w.to(dev)) for cid, w in waves.items()}


def case_sets(dev):
    c = concepts_on(dev)
    return [[c[i] for i in s] for s in CR.SETS]


def relerr(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / (np.abs(ref).max() + 1e-300))


def cosine(a, ref):
    return F.cosine_similarity(torch.as_tensor(np.asarray(a, np.float64)).flatten(), torch.as_tensor(ref).flatten(), dim=0).item()


@pytest.mark.parametrize("pool", ["none", "mean"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_tcav_parity_f32(gpu_device, stable, pool):
    tol, cmin = TOL["f32"]
    ref = CR.case_reference(stable, pool)
    tc = CO.HipTCAV(engine(gpu_device, "f32", stable), list(CR.LAYERS), pool=pool)
    out = tc.interpret(CR.case_inputs().to(gpu_device), case_sets(gpu_device))
    assert sorted(out) == sorted(ref) == ["0-1", "2-1"]
    for key in ref:
        for l in CR.LAYERS:
            r, o, cav = ref[key][l], out[key][l], tc.cavs[key][l]
            ew, cw = relerr(cav.weights.cpu().numpy(), r["weights"]), cosine(cav.weights.cpu().numpy(), r["weights"])
            es, cs = relerr(o["scores"].cpu().numpy(), r["scores"]), cosine(o["scores"].cpu().numpy(), r["scores"])
            em = float(np.abs(o["magnitude"].cpu().numpy() - r["magnitude"]).max() / np.abs(r["scores"]).max())
            print(f"[f32 {pool}] {key} layer {l}: CAV err {ew:.3e} cos {cw:.8f}; scores err {es:.3e} cos {cs:.8f}; magnitude err {em:.3e}; "
                  f"accs {cav.accs:.4f} / {r['accs']:.4f}; intercept err {np.abs(cav.intercepts - r['intercepts']).max():.3e}")
            assert tuple(cav.weights.shape) == r["weights"].shape and tuple(o["scores"].shape) == r["scores"].shape
            assert ew < tol and cw > cmin and es < tol and cs > cmin, (key, l)
            assert np.abs(r["scores"]).min() > 1e-3 * np.abs(r["scores"]).max()          # no reference score near zero: signs are decided
            assert (o["sign_count"].cpu().numpy() == r["sign_count"].astype(np.float32)).all()
            assert cav.accs == r["accs"] and em < tol and cav.classes == [int(k) for k in key.split("-")]


@pytest.mark.parametrize("pool", ["none", "mean"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_tcav_parity_f16(gpu_device, stable, pool):
    """The fp16-operand chain: scores within F16_SCORE_TOL of max|ref|; signs are compared outside a band of that width around
    zero, and at most 1 of the 8 inputs per (set, layer, concept) may fall inside it."""
    ref = CR.case_reference(stable, pool)
    tc = CO.HipTCAV(engine(gpu_device, "f16", stable), list(CR.LAYERS), pool=pool)
    out = tc.interpret(CR.case_inputs().to(gpu_device), case_sets(gpu_device))
    for key in ref:
        for l in CR.LAYERS:
            r, sc = ref[key][l], out[key][l]["scores"].cpu().numpy().astype(np.float64)
            scale = np.abs(r["scores"]).max()
            es = relerr(sc, r["scores"])
            inside = np.abs(r["scores"]) <= F16_SCORE_TOL * scale
            print(f"[f16 {pool}] {key} layer {l}: scores err {es:.3e}; CAV err {relerr(tc.cavs[key][l].weights.cpu().numpy(), r['weights']):.3e}; "
                  f"inside the band per concept {inside.sum(0)}")
            assert es < F16_SCORE_TOL, (key, l, es)
            assert (inside.sum(0) <= 1).all()
            assert ((sc > 0) == (r["scores"] > 0))[~inside].all()


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_last_layer_closed_form(gpu_device, stable):
    """At ``layer = nl`` (no final LayerNorm in the tiny model) the gradient is ``coef / T`` in every frame of every clip, so
    ``scores[b, c] = (1 / T) sum_t coef . w_c[t, :]`` from the returned CAV, for every b."""
    att = engine(gpu_device, "f32", stable)
    nl, H = att.eg.emb.nl, att.eg.cfg.hidden_size
    tc = CO.HipTCAV(att, [nl])
    out = tc.interpret(CR.case_inputs().to(gpu_device), case_sets(gpu_device)[:1])["0-1"][nl]
    W = tc.cavs["0-1"][nl].weights.cpu().double().view(2, -1, H)
    T = W.shape[1]
    coef = torch.as_tensor(CR.case_model(stable)[2], dtype=torch.float64).view(-1)
    expect = ((W @ coef).sum(1) / T)[None].expand(CR.N_INPUTS, 2).numpy()
    err = relerr(out["scores"].cpu().numpy(), expect)
    print(f"closed form at layer nl = {nl}: err {err:.3e}")
    assert err < TOL["f32"][0]


def test_chunking_sub_batch_and_negated_rows(gpu_device):
    att = engine(gpu_device, "f32")
    x, sets = CR.case_inputs().to(gpu_device), case_sets(gpu_device)
    runs = {}
    for chunk in (16, 5):                                                    # 12 clips per concept: one chunk, or 5 + 5 + 2
        tc = CO.HipTCAV(att, [4], internal_batch_size=chunk)
        runs[chunk] = (tc.interpret(x, sets), tc)
    a, tca = runs[16]
    for key in a:
        w = tca.cavs[key][4].weights
        assert torch.equal(w[0], -w[1])                                      # Captum's [-w, w]: exact negatives
        assert torch.equal(a[key][4]["scores"][:, 0], -a[key][4]["scores"][:, 1])
        b = runs[5][0][key][4]["scores"]
        # the chain is batch-invariant (tests/test_gpu_layer_attr.py asserts equal bits over its chunk sizes): so are these
        assert torch.equal(a[key][4]["scores"], runs[5][0][key][4]["scores"])
        assert torch.equal(tca.interpret(x[2:4], sets)[key][4]["scores"], a[key][4]["scores"][2:4])
        assert torch.equal(tca.interpret(x, sets)[key][4]["scores"], a[key][4]["scores"])     # a second call: the same bits


def test_shared_concept_runs_once_and_budget(gpu_device):
    att = engine(gpu_device, "f32")
    calls = []
    fwd = att.eg.forward
    att.eg.forward = lambda *a, **k: (calls.append(a[0].shape[0]), fwd(*a, **k))[1]
    try:
        tc = CO.HipTCAV(att, [0, 4], internal_batch_size=12)
        tc.compute_cavs(case_sets(gpu_device))
        assert calls == [12, 12, 12]                                         # three concepts in two sets, two layers: three forwards
        tc.compute_cavs(case_sets(gpu_device), force_train=True)
        assert calls == [12, 12, 12]
    finally:
        att.eg.forward = fwd
    with pytest.raises(MemoryError, match="memory_budget"):
        CO.HipTCAV(att, [0, 4], memory_budget=12 * 49 * 64 * 4).compute_cavs(case_sets(gpu_device))
    short = CO.Concept(5, "short", syn.make_clips(4, 8000, seed=1).to(gpu_device))
    with pytest.raises(ValueError, match="frame count"):
        CO.HipTCAV(att, [4]).compute_cavs([[concepts_on(gpu_device)[0], short]])
    cav = CO.HipTCAV(att, [4], pool="mean").compute_cavs([[concepts_on(gpu_device)[0], short]])["0-5"][4]     # lengths may differ
    assert tuple(cav.weights.shape) == (2, 64)


def test_frame_sensitivity_iterables_and_mean_difference(gpu_device):
    att = engine(gpu_device, "f32")
    x, sets = CR.case_inputs().to(gpu_device), case_sets(gpu_device)
    tc = CO.HipTCAV(att, [4], pool="mean")
    scores = tc.interpret(x, sets[:1])["0-1"][4]["scores"]
    fs = tc.frame_sensitivity(x, sets[0], 4)
    assert tuple(fs.shape) == (CR.N_INPUTS, 2, 49)
    total = fs.double().sum(2).cpu().numpy()
    g = att.layer_gradient_x_activation(x, 4, multiply_by_inputs=False).double().cpu()
    v = tc.cavs["0-1"][4].weights.double().cpu()
    bound = 49 * 2.0 ** -23 * (g.abs() @ v.abs().T).sum(1).max().item()     # fp32 summation of 49 x 64 terms, generously
    err = np.abs(total - scores.double().cpu().numpy()).max()
    print(f"frame_sensitivity summed over t vs the pooled score: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert relerr(fs.cpu().numpy(), torch.einsum("bth,ch->bct", g, v).numpy()) < 1e-5
    assert tuple(att.frames_to_wave(fs[:, 1].contiguous(), CR.L).shape) == (CR.N_INPUTS, CR.L)
    # Captum's data_iter: the same clips in batches of 5 give the same CAV
    waves = CR.case_concepts()
    it = [[CO.Concept(i, f"c{i}", [w.to(gpu_device) for w in waves[i].split(5)]) for i in (0, 1)]]
    w_it = CO.HipTCAV(att, [4], pool="mean", internal_batch_size=5).compute_cavs(it)["0-1"][4].weights
    w_t = CO.HipTCAV(att, [4], pool="mean", internal_batch_size=5).compute_cavs(sets[:1])["0-1"][4].weights
    assert torch.equal(w_it, w_t)
    md = CO.HipTCAV(att, [4], classifier="mean_difference").compute_cavs(sets[:1])["0-1"][4]
    acts = CO.HipTCAV(att, [4])
    feats = [acts._concept_activations(c)[4].double().cpu().numpy() for c in sets[0]]
    Wr, br, ar = CR.fit_cav(feats, classifier="mean_difference")
    assert relerr(md.weights.cpu().numpy(), Wr) < 1e-6 and md.accs == ar


class HostMeans(CO.Classifier):
    """A user classifier with Captum's protocol: the difference of the class means, computed on the host."""

    def train_and_eval(self, dataloader, **kwargs):
        xs, ys = zip(*[(x, y) for x, y in dataloader])
        x, y = torch.cat(xs).double(), torch.cat(ys)
        self.ids = sorted(set(y.tolist()))
        w = x[y == self.ids[1]].mean(0) - x[y == self.ids[0]].mean(0)
        self.w = torch.stack([-w, w]).float()
        return {"accs": torch.tensor(1.0)}

    def weights(self):
        return self.w

    def classes(self):
        return self.ids


def test_user_classifier_protocol(gpu_device):
    att = engine(gpu_device, "f32")
    sets = case_sets(gpu_device)[:1]
    user = CO.HipTCAV(att, [4], classifier=HostMeans()).compute_cavs(sets)["0-1"][4]
    ours = CO.HipTCAV(att, [4], classifier="mean_difference").compute_cavs(sets)["0-1"][4]
    assert user.classes == [0, 1] and user.accs == 1.0
    assert relerr(user.weights.cpu().numpy(), ours.weights.cpu().double().numpy()) < 1e-5


def test_range_contract(gpu_device):
    """A saturating activation (one FFN bias entry of 1e5, as tests/test_gpu_training.py) still raises SplitRangeError through
    compute_cavs, and the next valid call succeeds."""
    sd, cfg, coef, icpt = CR.case_model(False)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["encoder.layers.0.feed_forward.intermediate_dense.bias"][3] = 1e5
    bad = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision="f32"))
    with pytest.raises(_lib.SplitRangeError):
        CO.HipTCAV(bad, [4]).compute_cavs(case_sets(gpu_device)[:1])
    torch.cuda.synchronize()
    _lib.lib().advh_split_overflow(1)
    cav = CO.HipTCAV(engine(gpu_device, "f32"), [4]).compute_cavs(case_sets(gpu_device)[:1])["0-1"][4]
    assert bool(torch.isfinite(cav.weights).all())


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime, tmp_path):
    import captum_saliency as cs
    from captum.concept import TCAV, Concept
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    concepts = {i: Concept(i, f"c{i}", w.to(gpu_device)) for i, w in CR.case_concepts().items()}
    sets = [[concepts[i] for i in s] for s in CR.SETS]
    x = CR.case_inputs().to(gpu_device)
    front = TCAV(model, ["hidden_states.4", 0], save_path=str(tmp_path), model_id="tiny")
    out = front.interpret(x, sets)
    direct = CO.HipTCAV(eng, [4, 0]).interpret(x, sets)
    assert sorted(out) == ["0-1", "2-1"] and sorted(out["0-1"], key=str) == [0, "hidden_states.4"]
    for key in out:
        for name, l in (("hidden_states.4", 4), (0, 0)):
            for field in ("scores", "sign_count", "magnitude"):
                assert torch.equal(out[key][name][field], direct[key][l][field]), (key, name, field)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["tiny_0-1_layer0.npz", "tiny_0-1_layer4.npz", "tiny_2-1_layer0.npz", "tiny_2-1_layer4.npz"]
    again = TCAV(model, ["hidden_states.4", 0], save_path=str(tmp_path), model_id="tiny").compute_cavs(sets)     # reloaded from the files
    assert torch.equal(again["0-1"]["hidden_states.4"].weights, front.compute_cavs(sets)["0-1"]["hidden_states.4"].weights)
    norm = front.interpret(x, sets, magnitude="normalized")["0-1"]["hidden_states.4"]
    s = norm["scores"].double().cpu().numpy()
    assert np.allclose(norm["magnitude"].cpu().numpy(), np.abs(s * (s > 0)).sum(0) / np.abs(s).sum(0), rtol=1e-6)
    ig = TCAV(model, [4], layer_attr_method="integrated_gradients").interpret(x[:2], sets[:1], n_steps=4)["0-1"][4]["scores"]
    w4 = CO.HipTCAV(eng, [4]).compute_cavs(sets[:1])["0-1"][4].weights
    assert torch.equal(ig, CO.gram(eng.layer_integrated_gradients(x[:2], 4, n_steps=4).view(2, -1), w4).float())
    with pytest.raises(NotImplementedError):
        front.interpret(x, sets, target=1)
    with pytest.raises(ValueError):
        TCAV(model, ["hidden_states.10"])
