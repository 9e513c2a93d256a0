"""CPU-only: the argument contract of advh_attention_maps_long, advh_attention_bwd_value_long, advh_rollout_step_long and
advh_rollout_relevance_long (include/addvisor_hip.h).  ADVH_EINVAL and ADVH_EUNSUPPORTED come back before any HIP call, so they
can be exercised without a device.  Also the host logic of the ``long_maps`` opt-in: a bare chain (no workspace, no library
handle) gets as far as each check and no further, ``runtime`` reads ADDVISOR_LONG_MAPS when it builds its singleton and passes
the keyword only then, and ``lengths=`` on the four attribution methods needs the opt-in."""
import ctypes as C
import os
import re

import pytest
import torch

from addvisor_hip import _lib, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules
from test_attention_bwd_long_abi_cpu import bare_chain, bare_embedder

EINVAL, EUNSUPPORTED = -1, -4
NAMES = ("advh_attention_maps_long", "advh_attention_bwd_value_long", "advh_rollout_step_long", "advh_rollout_relevance_long")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    return C.addressof(buf), buf


def test_symbols_and_argtypes(lib):
    i, i64, vp, f = C.c_int, C.c_int64, C.c_void_p, C.c_float
    want = {"advh_attention_maps_long": (i, [vp, i64, vp, i64, f, i, vp, vp, vp, i, i, i, i, vp]),
            "advh_attention_bwd_value_long": (i, [vp, i64, vp, i64, vp, i64, vp, vp, i, i, i, i, vp]),
            "advh_rollout_step_long": (i, [vp, vp, vp, f, f, f, i, vp, i, i, vp]),
            "advh_rollout_relevance_long": (i, [vp, vp, vp, i, i, vp])}
    assert set(want) == set(NAMES)
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    root = os.path.join(os.path.dirname(_lib.CSRC), "..")
    header = open(os.path.join(root, "include", "addvisor_hip.h")).read()
    assert all(len(re.findall(rf"^int {name}\(", header, re.M)) == 1 for name in want)
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in integration for name in want)


def test_attention_maps_long_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_maps_long
    ok = dict(qkv=p, ql=0, dctx=p, dl=0, dscale=1.0, fuse=1, out=p, ws=p, frames=p, B=1, T=300, H=64, heads=1)
    call = lambda **kw: f(*(list({**ok, **kw}.values()) + [None]))
    for name in ("qkv", "out", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("B", "T", "H", "heads"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(heads=3) == EINVAL                                               # H % heads
    assert call(fuse=-1) == EINVAL and call(fuse=4) == EINVAL
    assert call(dscale=float("inf")) == EINVAL and call(dscale=float("nan")) == EINVAL
    assert call(ql=-8) == EINVAL and call(ql=4) == EINVAL
    assert call(dl=8) == EINVAL                                                  # fp16 qkv with split dctx
    assert call(ql=8, dl=0) == EINVAL and call(ql=8, dl=4) == EINVAL             # split qkv: dctx split too
    assert call(H=136) == EUNSUPPORTED and call(H=20) == EUNSUPPORTED            # head dim > 128, % 8
    assert call(H=272, heads=2) == EUNSUPPORTED and call(H=24, heads=2) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED                                         # one grid row per clip
    assert call(T=255 * 128 + 1) == EUNSUPPORTED                                 # 256 x 256 tiles of 128 x 128: the grid's z extent
    assert call(frames=None, B=65536) == EUNSUPPORTED                            # frames may be NULL: no EINVAL for it
    assert call(dctx=None, dl=12345, B=65536) == EUNSUPPORTED                    # dctx_lo is ignored without dctx
    assert call(qkv=None, H=136) == EINVAL and call(ws=None, B=65536) == EINVAL  # an argument error comes first


def test_attention_bwd_value_long_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_bwd_value_long
    ok = dict(qkv=p, ql=8, dctx=p, dl=8, dqkv=p, ol=8, ws=p, frames=p, B=1, T=300, H=64, heads=1)
    call = lambda **kw: f(*(list({**ok, **kw}.values()) + [None]))
    for name in ("qkv", "dctx", "dqkv", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("B", "T", "H", "heads"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(heads=3) == EINVAL
    for name in ("dl", "ol"):                                                    # split qkv: every tensor split
        assert call(**{name: 0}) == EINVAL and call(**{name: -8}) == EINVAL and call(**{name: 4}) == EINVAL, name
    assert call(ql=-8) == EINVAL and call(ql=12) == EINVAL
    assert call(ql=0) == EINVAL and call(ql=0, dl=0) == EINVAL                   # plain fp16 qkv: all plain
    assert call(ql=0, dl=0, ol=0, H=136) == EUNSUPPORTED
    assert call(H=136) == EUNSUPPORTED and call(H=20) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED and call(frames=None, T=65535 * 128 + 1) == EUNSUPPORTED
    assert call(ql=4, B=65536) == EINVAL and call(ws=None, H=136) == EINVAL


def test_rollout_long_arguments(lib, p):
    p, q = p[0], p[0] + 4096
    step = lib.advh_rollout_step_long
    ok = dict(M=p, X=q, Y=q + 4096, a=1.0, b=1.0, g=0.0, n=1, frames=p, B=1, T=300)
    call = lambda **kw: step(*(list({**ok, **kw}.values()) + [None]))
    for name in ("M", "X", "Y"):
        assert call(**{name: None}) == EINVAL, name
    assert call(Y=q) == EINVAL and call(Y=p) == EINVAL                           # Y == X, Y == M
    for name in ("B", "T"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(B=65536) == EUNSUPPORTED and call(frames=None, B=65536) == EUNSUPPORTED
    rel = lib.advh_rollout_relevance_long
    assert rel(None, p, p, 1, 300, None) == EINVAL and rel(p, None, p, 1, 300, None) == EINVAL
    assert rel(p, q, p, 0, 300, None) == EINVAL and rel(p, q, p, 1, 0, None) == EINVAL
    assert rel(p, q, None, 65536, 300, None) == EUNSUPPORTED


def test_whole_clip_entries_keep_their_limit(lib, p):
    p, q = p[0], p[0] + 4096
    assert lib.advh_attention_maps(p, 0, None, 0, 1.0, 0, p, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_bwd_value(p, 8, p, 8, p, 8, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_rollout_step(p, q, q + 4096, 1.0, 1.0, 0.0, 1, 1, 257, None) == EUNSUPPORTED
    assert lib.advh_rollout_relevance(p, q, 1, 257, None) == EUNSUPPORTED


def test_opt_in_is_off_by_default_and_needs_long_clips():
    assert EmbedderGrad.long_maps is False
    emb = bare_embedder(syn.tiny_config(False))
    with pytest.raises(ValueError, match="long_maps must be a bool"):
        EmbedderGrad(emb, long_clips=True, long_maps=1)
    with pytest.raises(ValueError, match="long_maps=True needs long_clips=True"):
        EmbedderGrad(emb, long_maps=True)
    with pytest.raises(ValueError, match="long_maps=True needs long_clips=True"):
        HipAttribution(emb, long_maps=True)
    with pytest.raises(ValueError, match="long_maps must be a bool"):
        HipAttribution(emb, long_clips=True, long_maps="yes")
    assert bare_chain(True).long_maps is False                                   # a bare chain that sets long_clips alone


def test_a_long_maps_chain_passes_the_frame_check_and_stops_at_the_next_step():
    """With long_maps the three calls get past the 256-frame refusal at 299 frames: the bare chain has no ``_rag``, so each
    fails where it first needs state.  Without it they refuse with the parent's text, now with the hint."""
    eg = bare_chain(True)
    eg._last = (None, 2, 96000, 96000)
    with pytest.raises(_lib.AdvhError, match=r"T x T attention kernels.*T <= 256 frames \(82319 samples\).*long_maps=True"):
        eg.attention_probs(0)
    eg.long_maps = True
    with pytest.raises(AttributeError):
        eg.attention_probs(0)
    with pytest.raises(AttributeError):
        eg.backward(to_layer=0, attention_maps=(torch.zeros(1), 1))
    with pytest.raises(AttributeError):
        eg.backward(to_layer=0, rules=LrpRules())


def test_runtime_passes_the_keyword_only_when_the_variable_is_set(monkeypatch):
    built = []

    class Old:                                                                   # a constructor from before the keyword
        def __init__(self, emb, precision=None, long_clips=False):
            built.append((long_clips, None))

    class New:
        def __init__(self, emb, precision=None, long_clips=False, long_maps=False):
            built.append((long_clips, long_maps))

    import addvisor_hip.embedder_grad as EG
    monkeypatch.setattr(runtime, "hip_embedder", lambda: None)
    monkeypatch.setenv("ADDVISOR_LONG_CLIPS", "1")
    for value in (None, "0", "", "false"):
        monkeypatch.setattr(EG, "EmbedderGrad", Old)
        if value is None:
            monkeypatch.delenv("ADDVISOR_LONG_MAPS", raising=False)
        else:
            monkeypatch.setenv("ADDVISOR_LONG_MAPS", value)
        runtime.reset()
        runtime.hip_embedder_grad()
        assert built[-1] == (True, None), value
    monkeypatch.setattr(EG, "EmbedderGrad", New)
    for value in ("1", "true"):
        monkeypatch.setenv("ADDVISOR_LONG_MAPS", value)
        runtime.reset()
        first = runtime.hip_embedder_grad()
        assert runtime.hip_embedder_grad() is first and built[-1] == (True, True), value
    monkeypatch.setenv("ADDVISOR_LONG_MAPS", "yes")
    runtime.reset()
    with pytest.raises(ValueError, match="ADDVISOR_LONG_MAPS must be 0 or 1"):
        runtime.hip_embedder_grad()
    monkeypatch.setenv("ADDVISOR_LONG_MAPS", "1")                                 # the real class: the variable needs ADDVISOR_LONG_CLIPS
    monkeypatch.setenv("ADDVISOR_LONG_CLIPS", "0")
    monkeypatch.setattr(EG, "EmbedderGrad", EmbedderGrad)
    monkeypatch.setattr(runtime, "hip_embedder", lambda: bare_embedder(syn.tiny_config(False)))
    runtime.reset()
    with pytest.raises(ValueError, match="long_maps=True needs long_clips=True"):
        runtime.hip_embedder_grad()
    runtime.reset()


class Stub:
    """An engine from before the feature: no ``long_maps`` attribute."""
    def __init__(self, emb):
        self.emb, self.cfg = emb, emb.cfg


def attribution(long_maps):
    emb = bare_embedder(syn.tiny_config(False))
    att = HipAttribution.__new__(HipAttribution)
    att.emb, att.eg = emb, Stub(emb)
    if long_maps is not None:
        att.eg.long_maps = long_maps
    att._prep = lambda waves: (_ for _ in ()).throw(AssertionError("_prep ran"))
    return att


@pytest.mark.parametrize("long_maps", [None, False])
def test_lengths_without_the_opt_in_raise_before_prep(long_maps):
    att = attribution(long_maps)
    w = torch.zeros(2, 16000)
    calls = (lambda: att.attention_maps(w, 0, lengths=[16000, 8000]), lambda: att.attention_rollout(w, lengths=[16000, 8000]),
             lambda: att.attention_grad_rollout(w, lengths=[16000, 8000]), lambda: att.transformer_lrp(w, lengths=[16000, 8000]))
    for call in calls:
        with pytest.raises(ValueError, match="lengths=.*long_maps=True"):
            call()
    with pytest.raises(ValueError, match="attention maps need T <= 256 frames"):  # the frame limit of an engine without the opt-in
        att.attention_rollout(torch.zeros(1, 82320))


def test_lengths_are_checked_before_prep_with_the_opt_in():
    att = attribution(True)
    with pytest.raises(ValueError, match=r"lengths"):
        att.attention_rollout(torch.zeros(2, 96000), lengths=[96000, 96001])
    with pytest.raises(AssertionError, match="_prep ran"):                        # 299 frames pass the frame check
        att.attention_rollout(torch.zeros(2, 96000))
