"""CPU-only: the restatement of conservative propagation (tests/lrp_ref.py) reduces to gradient x activation with its rules off,
conserves relevance on a bias-free model, and agrees with itself in fp64 far below the engine's bar; every argument check of the
engine and of the front end runs before any GPU work; the entry points of csrc/lrp.hip keep the header's error contract and
compile without scratch."""
import ctypes as C

import pytest
import torch

import attention_rollout_ref as AR
import lrp_ref as LR
from addvisor_hip import _lib, attribution as AT, synthetic as syn
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules
from test_build_resources import resources

torch.set_grad_enabled(False)

# The restatement in fp32 against itself in fp64, relative to max|ref| of each returned tensor: a tenth of the fp32-class bar of
# tests/test_gpu_lrp.py (1e-4), so that bar never measures the yardstick's own noise.
NOISE_FLOOR = 1e-5


def model_of(cfg):
    return (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))


def d120_config():
    return syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480, num_conv_pos_embedding_groups=2,
                           num_hidden_layers=10)


CASES = {"post_ln_1s": (lambda: syn.tiny_config(False), 2, 16000), "pre_ln_1s": (lambda: syn.tiny_config(True), 2, 16000),
         "post_ln_5s": (lambda: syn.tiny_config(False), 1, 80000), "pre_ln_5s": (lambda: syn.tiny_config(True), 1, 80000),
         "d120_1s": (d120_config, 2, 16000)}
RULES = {"default": dict(), "all_identity": dict(gelu_rule="identity"), "off": dict(ln_rule=False, attention_rule=False),
         "ln": dict(attention_rule=False), "attention": dict(ln_rule=False),
         "gelu": dict(ln_rule=False, attention_rule=False, gelu_rule="identity")}


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def _leaf(t):
    """The one leaf that requires grad in the autograd graph of ``t``."""
    seen, stack = set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if hasattr(fn, "variable"):
            return fn.variable
        stack.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no leaf")


def test_rules_off_is_gradient_x_activation():
    for name in ("post_ln_1s", "pre_ln_1s", "d120_1s"):
        mk, B, L = CASES[name]
        model = model_of(mk())
        x = syn.make_clips(B, L, seed=12)
        logits, _ = AR.encoder(x, model)
        h0 = _leaf(logits)
        with torch.enable_grad():
            (g,) = torch.autograd.grad(logits.sum(), h0)
        r = LR.explain(x, model, **RULES["off"])
        e_l, e_x, e_r = relerr(r["logits"], logits.detach()), relerr(r["x"], h0.detach()), relerr(r["R"], h0.detach() * g)
        print(f"{name}: rules off vs autograd gradient x activation of the rollout restatement's encoder (fp64): logits {e_l:.2e}, "
              f"x {e_x:.2e}, R {e_r:.2e}")
        assert e_l < 1e-12 and e_x < 1e-12 and e_r < 1e-12
        for rules in ("default", "all_identity"):                       # the rules change gradients, never a forward value
            assert relerr(LR.explain(x, model, **RULES[rules])["logits"], r["logits"]) < 1e-14       # x Phi(x) rounds unlike F.gelu
            assert relerr(LR.explain(x, model, **RULES[rules])["R"], r["R"]) > 1e-3


def test_conservation_without_biases():
    for name in ("post_ln_1s", "pre_ln_1s"):
        mk, B, L = CASES[name]
        model = LR.zero_bias_model(model_of(mk()))
        x = syn.make_clips(B, L, seed=12)
        for target, s0 in ((None, 0), (0, 0), (None, 4)):
            r = LR.explain(x, model, target=target, start_layer=s0, gelu_rule="identity")
            want = r["sign"] * r["logits"]
            gap = (r["rel"].sum(-1) - want).abs()
            mass = r["rel"].abs().sum(-1)
            print(f"{name} target={target} start_layer={s0}: |sum_t rel - (+-F)| {gap.tolist()} of sum_t |rel| {mass.tolist()}")
            assert bool((gap <= 1e-9 * mass).all())
        r = LR.explain(x, model)                                        # GELU's own gradient is not conservative
        assert bool(((r["rel"].sum(-1) - r["logits"]).abs() > 1e-6 * r["rel"].abs().sum(-1)).all())


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_noise_floor(name):
    mk, B, L = CASES[name]
    model = model_of(mk())
    x = syn.make_clips(B, L, seed=12)
    worst = {}
    for rules, s0 in (("default", 0), ("all_identity", 0), ("off", 0), ("ln", 4), ("attention", 4), ("gelu", 4)):
        kw = RULES[rules]
        r64, r32 = LR.explain(x, model, start_layer=s0, **kw), LR.explain(x, model, start_layer=s0, dtype=torch.float32, **kw)
        for k in ("rel", "R", "grad", "x", "logits"):
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64 and r32[k].shape == r64[k].shape
            worst[k] = max(worst.get(k, 0.0), relerr(r32[k], r64[k]))
    print(f"{name}: fp32 restatement vs fp64, max rel err of max|ref| per quantity over every rule set (start_layer 0 or 4): "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < NOISE_FLOOR, worst


def test_value_gradient_of_detached_probabilities_is_Pt_dO():
    g = torch.Generator().manual_seed(3)
    B, heads, T, d = 2, 3, 17, 8
    q, k, v, do = (torch.randn(B, heads, T, d, generator=g, dtype=torch.float64) for _ in range(4))
    with torch.enable_grad():
        q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
        P = torch.softmax(q @ k.transpose(2, 3) * d ** -0.5, -1)
        dq, dk, dv = torch.autograd.grad(((P.detach() @ v) * do).sum(), (q, k, v), allow_unused=True)
    assert dq is None and dk is None
    e = relerr(dv, P.detach().transpose(2, 3) @ do)
    print(f"dV of sg(P) V vs P^T dO: {e:.2e}")
    assert e < 1e-14


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
    for bad in (-1, 9, 10, 1.5, None, True, "0"):
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, start_layer=bad)
    for bad in ("Identity", "none", None, 1, True):
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, gelu_rule=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, ln_rule=bad)
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, attention_rule=bad)
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, return_hidden=bad)
    for bad in (2, -1, 1.0, "true", True, torch.tensor([0, 1, 1]), torch.tensor([0, 2]), torch.tensor([[0, 1]]), torch.tensor([True, False])):
        with pytest.raises(ValueError):
            eng.transformer_lrp(x, target=bad)
    with pytest.raises(ValueError):
        eng.transformer_lrp(torch.zeros(2, 3, 4))
    for e in (_Stub(T=257), _Stub(heads=3, hidden=36), _Stub(heads=1, hidden=136)):       # T > 256, head dim 12, head dim 136
        with pytest.raises(ValueError):
            e.transformer_lrp(x)
    for ok in (lambda: eng.transformer_lrp(x), lambda: eng.transformer_lrp(x, "predicted", 8, False, False, "identity", True),
               lambda: eng.transformer_lrp(x[0], target=torch.tensor([1])), lambda: _Stub(T=256).transformer_lrp(x, 0)):
        with pytest.raises(AssertionError):                           # valid arguments go on to the device
            ok()


def test_backward_validates_rules_before_any_launch():
    eg = object.__new__(EmbedderGrad)                                 # no device, no forward pass: the rule checks come first
    eg.emb = type("E", (), {"nl": 9})()
    for bad in (dict(rules="all"), dict(rules=(True, True, "gradient")), dict(rules=LrpRules()),               # no to_layer
                dict(rules=LrpRules(), to_layer=10), dict(rules=LrpRules(), to_layer=-1), dict(rules=LrpRules(), from_layer=3),
                dict(rules=LrpRules(), to_layer=2, from_layer=3), dict(rules=LrpRules(), from_layer=3, neuron=(0, 1, 1, 0, 1, 1))):
        with pytest.raises(ValueError):
            eg.backward(**bad)
    with pytest.raises(RuntimeError):                                 # valid: goes on to ask for the forward pass
        eg.backward(rules=LrpRules(False, True, "identity"), to_layer=0)
    for bad in (dict(ln=1), dict(attention=None), dict(gelu="Identity"), dict(gelu=None)):
        with pytest.raises(ValueError):
            LrpRules(**bad)
    r = LrpRules()
    assert (r.ln, r.attention, r.gelu) == (True, True, "gradient")
    with pytest.raises(Exception):
        r.ln = False                                                  # frozen


def test_explainer_knows_transformer_lrp():
    import captum_saliency as cs
    eng = _Stub()
    assert callable(cs._explainer(eng, "transformer_lrp")) and callable(cs._explainer(eng, "transformer_lrp", layer=4))
    assert callable(cs._explainer(eng, "transformer_lrp", nt_type="smoothgrad"))
    for bad in (-1, 9, 2.5, "4", True):
        with pytest.raises(ValueError):
            cs._explainer(eng, "transformer_lrp", layer=bad)
    with pytest.raises(AssertionError):
        cs._explainer(eng, "transformer_lrp")(torch.zeros(2, 16000))


def test_argument_errors_of_the_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    fb, fb2 = (C.c_float * 256)(), (C.c_float * 256)()
    p, p2 = C.addressof(fb), C.addressof(fb2)
    val = lambda qkv=p, qlo=4096, dctx=p, dlo=4096, dqkv=p2, olo=4096, B=1, T=16, H=64, heads=2: \
        lib.advh_attention_bwd_value(qkv, qlo, dctx, dlo, dqkv, olo, B, T, H, heads, None)
    for bad in (dict(qkv=None), dict(dctx=None), dict(dqkv=None), dict(B=0), dict(T=0), dict(heads=0), dict(H=0), dict(H=64, heads=3),
                dict(qlo=4), dict(qlo=-8), dict(dlo=0), dict(dlo=12), dict(olo=0), dict(olo=-8), dict(olo=20), dict(qlo=0),
                dict(qlo=0, dlo=0), dict(qlo=0, olo=0)):
        assert val(**bad) == EINVAL, bad
    for bad in (dict(T=257), dict(H=12, heads=1), dict(H=136, heads=1), dict(H=24, heads=2), dict(T=257, qlo=0, dlo=0, olo=0),
                dict(H=136, heads=1, qlo=0, dlo=0, olo=0)):
        assert val(**bad) == EUNSUPPORTED, bad
    ln = lambda x=p, x32=1, dy=p, dy32=1, g=p, add=None, of=p2, oh=None, M=4, Cc=32: \
        lib.advh_layernorm_bwd_frozen(x, x32, dy, dy32, g, add, of, oh, M, Cc, 1e-5, None)
    for bad in (dict(x=None), dict(dy=None), dict(g=None), dict(of=None), dict(M=0), dict(Cc=0), dict(Cc=30), dict(M=-1)):
        assert ln(**bad) == EINVAL, bad
    assert ln(Cc=2052) == EUNSUPPORTED
    lns = lambda x=p, x32=0, xlo=1024, dy=p, dy32=0, dlo=1024, g=p, add=None, of=None, oh=p2, olo=1024, M=4, Cc=32: \
        lib.advh_layernorm_bwd_frozen_split(x, x32, xlo, dy, dy32, dlo, g, add, of, oh, olo, M, Cc, 1e-5, None)
    for bad in (dict(x=None), dict(dy=None), dict(g=None), dict(oh=None), dict(M=0), dict(Cc=30), dict(xlo=0), dict(dlo=0), dict(olo=0),
                dict(xlo=6), dict(dlo=-4), dict(olo=1022)):
        assert lns(**bad) == EINVAL, bad
    assert lns(Cc=2052) == EUNSUPPORTED
    ge = lambda d=p, dlo=128, g1=p, glo=128, out=p2, olo=128, n=100: lib.advh_gelu_identity_bwd(d, dlo, g1, glo, out, olo, n, None)
    for bad in (dict(d=None), dict(g1=None), dict(out=None), dict(n=0), dict(n=-3), dict(dlo=-8), dict(dlo=64), dict(glo=0), dict(olo=99),
                dict(dlo=0), dict(dlo=0, glo=0)):
        assert ge(**bad) == EINVAL, bad


def test_lrp_kernels_do_not_spill():
    res = resources("lrp.hip")
    val = {k: v for k, v in res.items() if "attention_bwd_value_kernel" in k}
    assert len(val) == 12, sorted(res)                                # tiles 4 / 8 / 13 / 16 x head dims 32 / 64 / 128
    ln = {k: v for k, v in res.items() if "layernorm_bwd_frozen_kernel" in k}
    assert len(ln) == 12, sorted(res)                                 # x, dy fp32 or fp16-side x 2 / 4 / 8 vectors per lane
    ge = {k: v for k, v in res.items() if "gelu_identity_bwd_kernel" in k}
    assert len(ge) == 2, sorted(res)
    for k, v in {**val, **ln, **ge}.items():
        assert v["scratch"] == 0, (k, v)
