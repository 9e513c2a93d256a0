"""CPU-only: the argument contract of the ragged gradient chain's entry points (include/addvisor_hip.h): ADVH_EINVAL /
ADVH_EUNSUPPORTED come back before any HIP call, so they can be exercised without a device.  Also the Python argument errors of
``EmbedderGrad`` and ``HipAttribution`` with ``lengths``, all raised on the host before anything is allocated."""
import ctypes as C
import inspect

import pytest
import torch

from addvisor_hip import _lib, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    return C.addressof(buf), buf


def test_attention_bwd_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_bwd_f16_ragged
    ok = [p, p, p, p, 1, 16, 64, 1, None]                                        # qkv, dctx, dqkv, frames, B, T, H, heads
    for i in range(4):                                                           # every pointer, frames included
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    for i, bad in ((4, 0), (5, 0), (6, 0), (7, 0), (7, 3), (4, -1)):             # B, T, H, heads <= 0, H % heads
        assert f(*[bad if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, bad)
    assert f(p, p, p, p, 1, 257, 64, 1, None) == EUNSUPPORTED                    # T > 256
    assert f(p, p, p, p, 1, 16, 136, 1, None) == EUNSUPPORTED and f(p, p, p, p, 1, 16, 20, 1, None) == EUNSUPPORTED     # head dim > 128, % 8
    assert lib.advh_attention_bwd_f16(p, p, p, 1, 257, 64, 1, None) == EUNSUPPORTED          # the sibling answers the same way
    g = lib.advh_attention_bwd_split_ragged
    ok = [p, 8, p, 8, p, 8, p, 1, 16, 64, 1, None]                               # qkv, lo, dctx, lo, dqkv, lo, frames, B, T, H, heads
    for i in (0, 2, 4, 6):
        assert g(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    for i in (1, 3, 5):                                                          # no lo plane, a plane distance % 8
        for bad in (0, -8, 4, 12):
            assert g(*[bad if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, bad)
    for i, bad in ((7, 0), (8, 0), (9, 0), (10, 0), (10, 3)):
        assert g(*[bad if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, bad)
    assert g(p, 8, p, 8, p, 8, p, 1, 257, 64, 1, None) == EUNSUPPORTED and g(p, 8, p, 8, p, 8, p, 1, 16, 136, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_bwd_split(p, 8, p, 8, p, 8, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_bwd_split(p, 4, p, 8, p, 8, 1, 16, 64, 1, None) == EINVAL


def test_row_kernels_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_pool_logreg_bwd_ragged
    ok = [p, p, p, p, p, 1, 4, 64, None]                                         # coef, dlogit, dh, dh16, frames, B, T, H
    for i in (0, 1, 4):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    assert f(p, p, None, None, p, 1, 4, 64, None) == EINVAL                      # no output at all (one of the two may be absent)
    for i, bad in ((5, 0), (6, 0), (7, 0), (7, 6)):                              # B, T, H <= 0, H % 4
        assert f(*[bad if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, bad)
    g = lib.advh_pool_logreg_bwd_split_ragged
    ok = [p, p, p, p, 8, p, 1, 4, 64, None]
    for i in (0, 1, 5):
        assert g(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    assert g(p, p, p, p, 0, p, 1, 4, 64, None) == EINVAL and g(p, p, p, p, 6, p, 1, 4, 64, None) == EINVAL     # a bad plane distance
    assert g(p, p, None, None, 8, p, 1, 4, 64, None) == EINVAL and g(p, p, p, p, 8, p, 1, 4, 6, None) == EINVAL
    z = lib.advh_zero_tail_rows_h
    assert z(None, 0, p, 1, 4, 64, None) == EINVAL and z(p, 0, None, 1, 4, 64, None) == EINVAL and z(p, -8, p, 1, 4, 64, None) == EINVAL
    assert z(p, 0, p, 0, 4, 64, None) == EINVAL and z(p, 0, p, 1, 0, 64, None) == EINVAL and z(p, 0, p, 1, 4, 0, None) == EINVAL
    assert z(p, 0, p, 65536, 4, 64, None) == EUNSUPPORTED and lib.advh_zero_tail_rows(p, p, 65536, 4, 64, None) == EUNSUPPORTED


def gn0_args(p, **kw):
    a = dict(wave=p, stride=4000, n_in=4000, B=1, L=4000, w0=p, gamma=p, stats=p, norm=p, mr=p, dy=p, dy_lo=1 << 20, part=p, sums=p, dz=p,
             dz_lo=1 << 20, T0=799, P0=800, C0=32, lens=p)
    a.update(kw)
    return a


def call_gn0(lib, split, a):
    head = (a["wave"], a["stride"], a["n_in"], a["B"], a["L"], a["w0"], a["gamma"], a["stats"], a["norm"], a["mr"], a["dy"])
    if split:
        return lib.advh_w2v2_frontend_bwd_group_split_ragged(*head, a["dy_lo"], a["part"], a["sums"], a["dz"], a["dz_lo"], a["T0"], a["P0"],
                                                             a["C0"], a["lens"], None)
    return lib.advh_w2v2_frontend_bwd_group_ragged(*head, a["part"], a["sums"], a["dz"], a["T0"], a["P0"], a["C0"], a["lens"], None)


@pytest.mark.parametrize("split", [False, True])
def test_frontend_bwd_group_ragged_arguments(lib, p, split):
    p = p[0]
    bad = [dict(lens=None), dict(wave=None), dict(w0=None), dict(gamma=None), dict(stats=None), dict(norm=None), dict(mr=None), dict(dy=None),
           dict(part=None), dict(sums=None), dict(dz=None), dict(B=0), dict(L=9), dict(n_in=0), dict(C0=0), dict(C0=31), dict(C0=514),
           dict(T0=798), dict(P0=798)]
    if split:
        bad += [dict(dy_lo=0), dict(dz_lo=0), dict(dy_lo=3), dict(dz_lo=-2)]
    for kw in bad:
        assert call_gn0(lib, split, gn0_args(p, **kw)) == EINVAL, kw


def test_wave_bwd_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_wave_bwd_ragged
    ok = [p, p, 4000, 4000, 1, 4000, p, p, p, 1, 1.0, p, 4000, 799, 800, p, None]   # g, wave, stride, n_in, B, L, stats, dxhat, part, normalize, scale, dx, dx_stride, T0, P0, lens
    for i in (0, 1, 6, 7, 8, 11, 15):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    for i, bad in ((3, 0), (4, 0), (5, 0), (5, 9), (12, 3999), (13, 798), (14, 798)):
        assert f(*[bad if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, bad)


# ------------------------------------------------------------------------------------------------ the Python argument errors
def bare_chain(stable=True):
    """An EmbedderGrad without a device: the host checks run before anything touches one."""
    cfg = syn.tiny_config(stable)
    emb = HipEmbedder.__new__(HipEmbedder)
    emb.cfg, emb.nl = cfg, min(cfg.layer_index, cfg.num_hidden_layers)
    eg = EmbedderGrad.__new__(EmbedderGrad)
    eg.emb, eg.cfg, eg._ws, eg._rag, eg._stop, eg._start = emb, cfg, {}, None, None, None
    return eg


def test_lengths_are_checked_before_anything_is_allocated():
    eg = bare_chain()
    w = torch.zeros(3, 4321)                                                     # a host tensor: reaching a launch would fail differently
    with pytest.raises(ValueError, match="not both"):
        eg.forward(w, length=4321, lengths=[4321, 400, 400])
    for bad in ([4321, 400], [4321, 400.0, 400], [4321, 4322, 400], [4321, 399, 400], torch.tensor([4321.0, 400.0, 400.0]), 5):
        with pytest.raises(ValueError):
            eg.forward(w, lengths=bad)
    with pytest.raises(ValueError, match=r"clip 1 has 399 samples.*shortest supported length is 400"):
        eg.forward(w, lengths=[4321, 399, 400])
    assert eg._ws == {} and eg._rag is None
    att = HipAttribution.__new__(HipAttribution)
    att.emb, att.eg = eg.emb, eg
    for call in (att.input_gradient, att.saliency, att.input_x_gradient, att.logits, att.integrated_gradients):
        with pytest.raises(ValueError, match="exceeds"):
            call(w, lengths=[4321, 4322, 400])
        with pytest.raises(ValueError, match="2 entries for a batch of 3"):
            call(w, lengths=[4321, 400])
    assert att._lens is None and eg._ws == {}


def test_out_of_scope_arguments_after_a_ragged_pass():
    """attention_maps / rules -> ValueError, forward_from -> RuntimeError, before any launch: the chain has no device here."""
    eg = bare_chain()
    eg._last = (None, 3, 4321, 4321)                                             # as a ragged pass leaves it
    eg._rag = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="attention_maps"):
        eg.backward(to_layer=0, attention_maps=(torch.zeros(1, 3, 13, 13), 1))
    with pytest.raises(ValueError, match="rules"):
        eg.backward(to_layer=0, rules=LrpRules())
    with pytest.raises(RuntimeError, match="ragged"):
        eg.forward_from(0, torch.zeros(3, 13, 32))
    with pytest.raises(ValueError, match="ragged"):
        eg.attention_probs(0)
    assert eg._ws == {}


def test_signatures():
    assert inspect.signature(EmbedderGrad.forward).parameters["lengths"].default is None
    for fn in (HipAttribution.input_gradient, HipAttribution.saliency, HipAttribution.input_x_gradient, HipAttribution.logits,
               HipAttribution.integrated_gradients):
        assert inspect.signature(fn).parameters["lengths"].default is None
    for fn in (HipAttribution.gradient_shap, HipAttribution.occlusion, HipAttribution.feature_ablation):
        assert "lengths" not in inspect.signature(fn).parameters                 # every other method is unchanged
    assert list(inspect.signature(EmbedderGrad.backward).parameters)[1:] == [
        "loss_scale", "seed", "to_layer", "from_layer", "neuron", "layer_seed", "row_scale", "attention_maps", "rules"]
