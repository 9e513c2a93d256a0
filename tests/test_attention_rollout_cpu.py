"""CPU-only: the restatement of the attention maps and rollouts (tests/attention_rollout_ref.py) agrees with the oracle and
with itself in fp64 far below the engine's bar, has the properties the definitions promise, every argument check of the engine
and of the front end runs before any GPU work, and the three entry points of csrc/attention_maps.hip keep the header's error
contract and compile without scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_rollout_ref as AR
from addvisor_hip import _lib, attribution as AT, synthetic as syn
from oracle import wav2vec2_ref as W
from test_build_resources import resources

torch.set_grad_enabled(False)

# The restatement in fp32 against itself in fp64, relative to max|ref| of each returned tensor: a tenth of the fp32-class bar of
# tests/test_gpu_attention_rollout.py (1e-4), so that bar never measures the yardstick's own noise.
NOISE_FLOOR = 1e-5


def model_of(cfg):
    return (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))


def d120_config():
    return syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480, num_conv_pos_embedding_groups=2,
                           num_hidden_layers=10)


CASES = {"post_ln_1s": (lambda: syn.tiny_config(False), 2, 16000, 49), "pre_ln_1s": (lambda: syn.tiny_config(True), 2, 16000, 49),
         "post_ln_2s": (lambda: syn.tiny_config(False), 2, 32000, 99), "pre_ln_2s": (lambda: syn.tiny_config(True), 2, 32000, 99),
         "post_ln_5s": (lambda: syn.tiny_config(False), 1, 80000, 249), "pre_ln_5s": (lambda: syn.tiny_config(True), 1, 80000, 249),
         "d120_1s": (d120_config, 2, 16000, 49), "base_1s": (syn.base_config, 1, 16000, 49)}
_REF = {}


def ref_of(name, target=None):
    """The fp64 restatement of a case, computed once."""
    key = (name, str(target))
    if key not in _REF:
        mk, B, L, T = CASES[name]
        model = model_of(mk())
        x = syn.make_clips(B, L, seed=12)
        _REF[key] = (model, x, AR.explain(x, model, target=target))
    return _REF[key]


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def tensors(r):
    """Every returned quantity as (name, tensor), the per-layer ones layer by layer."""
    for k in ("A", "G", "G_ctx", "GA", "Abar"):
        for l, t in enumerate(r[k]):
            yield f"{k}[{l}]", t
    for f in AR.FUSIONS:
        yield f"R[{f}]", r["R"][f]
        yield f"rel[{f}]", r["rel"][f]
    yield "D", r["D"]
    yield "rel_grad", r["rel_grad"]
    yield "logits", r["logits"]


def test_restated_encoder_is_the_oracle_classifier():
    for name in ("post_ln_1s", "pre_ln_1s"):
        model, x, r = ref_of(name)
        ref = W.classify(x, *model)[0].view(-1)
        d = (r["logits"].float() - ref).abs().max().item()
        print(f"{name}: restated fp64 logits vs oracle fp32 classify: {d:.3e}")
        assert d < 1e-5
        nl, heads, T = AR.num_layers(model[1]), model[1].num_attention_heads, CASES[name][3]
        assert len(r["A"]) == nl == 9 and tuple(r["A"][0].shape) == (x.shape[0], heads, T, T)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_noise_floor(name):
    model, x, r64 = ref_of(name)
    r32 = AR.explain(x, model, dtype=torch.float32)
    worst = {}
    for (k, a), (_, b) in zip(tensors(r32), tensors(r64)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
        q = k.split("[")[0]
        worst[q] = max(worst.get(q, 0.0), relerr(a, b))
    print(f"{name}: fp32 restatement vs fp64, max rel err of max|ref| per quantity (per layer for the maps): "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < NOISE_FLOOR, worst


def test_gradient_at_the_probabilities_is_dO_Vt():
    for name in ("post_ln_1s", "pre_ln_1s", "d120_1s"):
        _, _, r = ref_of(name)
        for l, (g, gc) in enumerate(zip(r["G"], r["G_ctx"])):
            assert relerr(gc, g) < 1e-12, (name, l)


def test_plain_rollout_rows_sum_to_one():
    for name in ("post_ln_1s", "pre_ln_2s"):
        _, _, r = ref_of(name)
        for f in AR.FUSIONS:
            R, rel = r["R"][f], r["rel"][f]
            assert (R >= 0).all()
            assert (R.sum(-1) - 1).abs().max().item() < 1e-12 and (rel.sum(-1) - 1).abs().max().item() < 1e-12, (name, f)
        A = r["A"]
        one = (0.5 * AR.fuse_heads(A[-1], "mean") + 0.5 * torch.eye(A[-1].shape[-1], dtype=A[-1].dtype))
        assert relerr(AR.rollout(A, "mean", start_layer=len(A) - 1), one) < 1e-12          # "mean": 0.5 A + 0.5 I per layer


def test_gradient_rollout_properties():
    for name in ("post_ln_1s", "pre_ln_1s"):
        _, _, r1 = ref_of(name, 1)
        _, _, r0 = ref_of(name, 0)
        _, _, rn = ref_of(name)
        assert (r1["D"] >= 0).all() and (r0["D"] >= 0).all()
        assert torch.equal(r1["D"], rn["D"])                                               # target=None explains +F
        for l in range(len(r1["A"])):
            assert torch.equal(r1["A"][l], r0["A"][l])
            lhs, rhs = r1["Abar"][l] - r0["Abar"][l], (r1["G"][l] * r1["A"][l]).mean(1)    # x^+ - (-x)^+ = x
            assert relerr(lhs, rhs) < 1e-12, (name, l)


def test_targets():
    model, x, r = ref_of("post_ln_1s")
    sign = torch.sign(r["logits"])
    pred = AR.explain(x, model, target="predicted")
    mixed = AR.explain(x, model, target=torch.tensor([0, 1]))
    r0, r1 = ref_of("post_ln_1s", 0)[2], ref_of("post_ln_1s", 1)[2]
    for b in range(2):
        want = r1 if sign[b] > 0 else r0
        assert relerr(pred["Abar"][0][b], want["Abar"][0][b]) < 1e-12
        assert relerr(mixed["Abar"][0][b], (r0, r1)[b]["Abar"][0][b]) < 1e-12


def test_start_layer_is_the_product_over_the_upper_layers():
    model, x, r = ref_of("pre_ln_1s")
    s = 4
    rs = AR.explain(x, model, start_layer=s)
    T = r["A"][0].shape[-1]
    eye = torch.eye(T, dtype=torch.float64)
    for f in AR.FUSIONS:
        prod = eye.expand(2, T, T)
        for a in r["A"][s:]:
            M = AR.fuse_heads(a, f)
            prod = ((eye + M) / (1 + M.sum(-1, keepdim=True))) @ prod
        assert relerr(rs["R"][f], prod) < 1e-12
    prod = eye.expand(2, T, T)
    for ab in r["Abar"][s:]:
        prod = (eye + ab) @ prod
    assert relerr(rs["D"], prod - eye) < 1e-9
    assert not torch.equal(rs["D"], r["D"])


class _Stub(AT.HipAttribution):
    def __init__(self, T=49, heads=2, hidden=64):
        class E:
            nl = 9
            cfg = type("Cfg", (), {"hidden_size": hidden, "num_attention_heads": heads})()

            def _lengths(self, L):
                return [T]
        self.eg = type("G", (), {"emb": E()})()

    def _prep(self, waves):
        raise AssertionError("the engine reached the device before rejecting its arguments")


def test_engine_validates_before_gpu_work():
    eng = _Stub()
    x = torch.zeros(2, 16000)
    for bad in (-1, 9, 10, 1.5, None, True, "0"):                     # layer nl has no attention block
        with pytest.raises(ValueError):
            eng.attention_maps(x, bad)
        with pytest.raises(ValueError):
            eng.attention_rollout(x, start_layer=bad)
        with pytest.raises(ValueError):
            eng.attention_grad_rollout(x, start_layer=bad)
    for bad in ("sum", "Mean", 1, 0, True):
        with pytest.raises(ValueError):
            eng.attention_maps(x, 0, head_fusion=bad)
        with pytest.raises(ValueError):
            eng.attention_rollout(x, head_fusion=bad)
    with pytest.raises(ValueError):
        eng.attention_rollout(x, head_fusion=None)                    # a rollout needs one matrix per layer
    for bad in (2, -1, 1.0, "true", True, torch.tensor([0, 1, 1]), torch.tensor([0, 2]), torch.tensor([[0, 1]]),
                torch.tensor([True, False])):
        with pytest.raises(ValueError):
            eng.attention_maps(x, 0, grad=True, target=bad)
        with pytest.raises(ValueError):
            eng.attention_grad_rollout(x, target=bad)
    with pytest.raises(ValueError):
        eng.attention_maps(x, 0, target=1)                            # a target without grad=True
    with pytest.raises(ValueError):
        eng.attention_maps(x, 0, grad=1)
    with pytest.raises(ValueError):
        eng.attention_maps(torch.zeros(2, 3, 4), 0)
    for e in (_Stub(T=257), _Stub(heads=3, hidden=36), _Stub(heads=1, hidden=136)):       # T > 256, head dim 12, head dim 136
        for fn in (lambda: e.attention_maps(x, 0), lambda: e.attention_rollout(x), lambda: e.attention_grad_rollout(x)):
            with pytest.raises(ValueError):
                fn()
    for ok in (lambda: eng.attention_maps(x, 8), lambda: eng.attention_maps(x, 0, "max", True, "predicted"),
               lambda: eng.attention_maps(x, 0, grad=True, target=torch.tensor([0, 1])), lambda: eng.attention_rollout(x, "min", 8),
               lambda: eng.attention_grad_rollout(x, 0, 4), lambda: eng.attention_grad_rollout(x[0], np.int64(1))):
        with pytest.raises(AssertionError):                           # valid arguments go on to the device
            ok()


def test_check_helpers():
    assert [AT.check_head_fusion(f) for f in (None, "mean", "max", "min")] == [0, 1, 2, 3]
    assert AT.check_attention_target(None, 2) is None and AT.check_attention_target(1, 2) is None
    assert AT.check_attention_target("predicted", 2) == "predicted"
    assert AT.check_attention_target(0, 3).tolist() == [-1.0, -1.0, -1.0]
    assert AT.check_attention_target(torch.tensor([1, 0]), 2).tolist() == [1.0, -1.0]


def test_explainer_knows_the_rollouts():
    import captum_saliency as cs
    eng = _Stub()
    for method in ("attention_rollout", "attention_grad_rollout"):
        assert callable(cs._explainer(eng, method)) and callable(cs._explainer(eng, method, layer=4))
        assert callable(cs._explainer(eng, method, nt_type="smoothgrad"))              # NoiseTunnel wraps [R, L] -> [R, L] methods
        for bad in (-1, 9, 2.5, "4", True):
            with pytest.raises(ValueError):
                cs._explainer(eng, method, layer=bad)
        with pytest.raises(AssertionError):
            cs._explainer(eng, method)(torch.zeros(2, 16000))


def test_argument_errors_of_the_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    fb = (C.c_float * 256)()
    fb2 = (C.c_float * 256)()
    p, p2 = C.addressof(fb), C.addressof(fb2)
    maps = lambda qkv=p, qlo=4096, dctx=p, dlo=4096, ds=1.0, fuse=0, out=p2, B=1, T=16, H=64, heads=2: \
        lib.advh_attention_maps(qkv, qlo, dctx, dlo, ds, fuse, out, B, T, H, heads, None)
    for bad in (dict(qkv=None), dict(out=None), dict(B=0), dict(T=0), dict(heads=0), dict(H=64, heads=3), dict(fuse=4), dict(fuse=-1),
                dict(qlo=4), dict(qlo=-8), dict(dlo=0), dict(dlo=12), dict(qlo=0), dict(ds=float("inf")), dict(ds=float("nan"))):
        assert maps(**bad) == EINVAL, bad
    for bad in (dict(T=257), dict(H=12, heads=1), dict(H=136, heads=1), dict(H=24, heads=2), dict(T=257, dctx=None),
                dict(H=136, heads=1, qlo=0, dlo=0)):
        assert maps(**bad) == EUNSUPPORTED, bad
    step = lambda M=p, X=p, Y=p2, B=1, T=8, a=1.0, b=1.0, g=0.0, n=1: lib.advh_rollout_step(M, X, Y, a, b, g, n, B, T, None)
    for bad in (dict(M=None), dict(X=None), dict(Y=None), dict(Y=p), dict(X=p2, Y=p2), dict(B=0), dict(T=0), dict(T=-1)):
        assert step(**bad) == EINVAL, bad
    assert step(T=257) == EUNSUPPORTED
    rel = lambda X=p, r=p2, B=1, T=8: lib.advh_rollout_relevance(X, r, B, T, None)
    for bad in (dict(X=None), dict(r=None), dict(B=0), dict(T=0)):
        assert rel(**bad) == EINVAL, bad
    assert rel(T=257) == EUNSUPPORTED


def test_attention_maps_kernels_do_not_spill():
    res = resources("attention_maps.hip")
    maps = {k: v for k, v in res.items() if "attention_maps_kernel" in k}
    assert len(maps) == 24, sorted(res)                               # tiles 4 / 8 / 13 / 16 x head dims 32 / 64 / 128 x grad or not
    rest = {k: v for k, v in res.items() if "rollout_step_kernel" in k or "rollout_relevance_kernel" in k}
    assert len(rest) == 2, sorted(res)
    for k, v in {**maps, **rest}.items():
        assert v["scratch"] == 0, (k, v)
