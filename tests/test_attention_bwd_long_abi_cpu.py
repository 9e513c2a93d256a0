"""CPU-only: the argument contract of advh_attention_bwd_long_f16 / advh_attention_bwd_long_split and
advh_attention_bwd_long_ws_bytes (include/addvisor_hip.h).  ADVH_EINVAL and ADVH_EUNSUPPORTED come back before any HIP call, so
they can be exercised without a device.  Also the host logic of the ``long_clips`` opt-in of the gradient chain: a bare chain
(no workspace, no library handle, CPU tensors) gets as far as each check and no further, and ``runtime`` reads
ADDVISOR_LONG_CLIPS when it builds its singleton."""
import ctypes as C
import os
import re

import pytest
import torch

import attention_bwd_long_cases as cases
from addvisor_hip import _lib, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, LrpRules, check_chain_frames

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    return C.addressof(buf), buf


def test_symbols_and_argtypes(lib):
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    want = {"advh_attention_bwd_long_ws_bytes": (C.c_size_t, [i, i, i]),
            "advh_attention_bwd_long_f16": (i, [vp, vp, vp, vp, vp, i, i, i, i, vp]),
            "advh_attention_bwd_long_split": (i, [vp, i64, vp, i64, vp, i64, vp, vp, i, i, i, i, vp])}
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "addvisor_hip.h")).read()
    assert all(len(re.findall(rf"^(?:int|size_t) {name}\(", header, re.M)) == 1 for name in want)


def test_workspace_bytes(lib):
    f = lib.advh_attention_bwd_long_ws_bytes
    for B, T, heads in ((1, 1, 1), (2, 273, 2), (16, 499, 12), (3, 513, 3), (40, 199, 16)):
        exact = 3 * B * heads * T * 4
        assert f(B, T, heads) == -(-exact // 256) * 256 == cases.ws_bytes(B, T, heads), (B, T, heads)
        assert exact <= f(B, T, heads) < exact + 256
    assert f(0, 5, 1) == 0 and f(1, 0, 1) == 0 and f(1, 5, -1) == 0
    assert f(65535, 65535 * 128, 16) == -(-3 * 65535 * 16 * 65535 * 128 * 4 // 256) * 256       # size_t: no 32-bit wrap


def test_attention_bwd_long_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_bwd_long_f16
    ok = dict(qkv=p, dctx=p, dqkv=p, ws=p, frames=p, B=1, T=300, H=64, heads=1)
    call = lambda **kw: f(*(list({**ok, **kw}.values()) + [None]))
    for name in ("qkv", "dctx", "dqkv", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("B", "T", "H", "heads"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(heads=3) == EINVAL                                               # H % heads
    assert call(H=136) == EUNSUPPORTED and call(H=20) == EUNSUPPORTED            # head dim > 128, % 8
    assert call(H=272, heads=2) == EUNSUPPORTED and call(H=24, heads=2) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED                                         # one grid row per clip
    assert call(T=65535 * 128 + 1) == EUNSUPPORTED                               # 65 536 blocks of 128 rows
    assert call(frames=None, B=65536) == EUNSUPPORTED                            # frames may be NULL: no EINVAL for it
    assert call(qkv=None, H=136) == EINVAL                                       # an argument error comes first
    g = lib.advh_attention_bwd_long_split
    ok = dict(qkv=p, ql=8, dctx=p, dl=8, dqkv=p, ol=8, ws=p, frames=p, B=1, T=300, H=64, heads=1)
    call = lambda **kw: g(*(list({**ok, **kw}.values()) + [None]))
    for name in ("qkv", "dctx", "dqkv", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("B", "T", "H", "heads"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(heads=3) == EINVAL
    for name in ("ql", "dl", "ol"):                                              # no lo plane, a negative or a misaligned distance
        assert call(**{name: 0}) == EINVAL and call(**{name: -8}) == EINVAL and call(**{name: 4}) == EINVAL and call(**{name: 12}) == EINVAL, name
    assert call(H=136) == EUNSUPPORTED and call(H=20) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED and call(frames=None, T=65535 * 128 + 1) == EUNSUPPORTED
    assert call(ql=4, B=65536) == EINVAL


def test_whole_clip_backward_entries_keep_their_limit(lib, p):
    p = p[0]
    assert lib.advh_attention_bwd_f16(p, p, p, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_bwd_split(p, 8, p, 8, p, 8, 1, 257, 64, 1, None) == EUNSUPPORTED


def bare_embedder(cfg):
    emb = HipEmbedder.__new__(HipEmbedder)                                        # the host checks need no device
    emb.cfg = cfg
    emb.nl = min(cfg.layer_index, cfg.num_hidden_layers)
    return emb


def bare_chain(long_clips):
    emb = bare_embedder(syn.tiny_config(False))
    eg = EmbedderGrad.__new__(EmbedderGrad)
    eg.emb, eg.cfg, eg.split = emb, emb.cfg, False
    if long_clips is not None:
        eg.long_clips = long_clips
    return eg


def test_opt_in_is_off_by_default_and_the_refusal_says_how():
    assert EmbedderGrad.long_clips is False
    emb = bare_embedder(syn.tiny_config(False))
    check_chain_frames(emb, 96000, True)                                         # opted in: no refusal
    check_chain_frames(emb, 82319)
    check_chain_frames(emb, 82319, True)
    for eg in (bare_chain(None), bare_chain(False)):
        with pytest.raises(_lib.AdvhError, match=r"256 frames \(82319 samples\).*T = 299 \(96000 samples\).*forward-only.*long_clips=True"):
            eg.forward(torch.zeros(2, 96000))
    with pytest.raises(ValueError, match="long_clips must be a bool"):
        EmbedderGrad(emb, long_clips=1)
    with pytest.raises(TypeError):
        HipAttribution(emb, long_clips=True, nonsense=1)


def test_a_long_chain_passes_the_frame_check_and_stops_at_the_next_step():
    """With long_clips the host check lets 299 frames through: the bare chain then fails where it first needs a workspace, not
    with the refusal."""
    eg = bare_chain(True)
    with pytest.raises(AttributeError):
        eg.forward(torch.zeros(2, 96000))


def test_maps_probs_and_rules_keep_the_256_frame_limit():
    """Above 256 frames attention_maps=, attention_probs and rules= raise on the host, naming the limit of the T x T kernels: the
    bare chain has no workspace, no ``_rag`` and no library handle, so any step further would fail differently."""
    eg = bare_chain(True)
    eg._last = (None, 2, 96000, 96000)
    pat = r"T x T attention kernels.*T <= 256 frames \(82319 samples\).*T = 299 \(96000 samples\)"
    with pytest.raises(_lib.AdvhError, match=r"attention_probs.*" + pat):
        eg.attention_probs(0)
    with pytest.raises(_lib.AdvhError, match=r"attention_maps.*" + pat):
        eg.backward(to_layer=0, attention_maps=(torch.zeros(1), 1))
    with pytest.raises(_lib.AdvhError, match=r"rules.*" + pat):
        eg.backward(to_layer=0, rules=LrpRules())
    eg._last = (None, 2, 82319, 82319)                                           # 256 frames: the check passes, the next step needs state
    with pytest.raises(AttributeError):
        eg.attention_probs(0)


def test_runtime_reads_the_switch_when_it_builds_the_singleton(monkeypatch):
    built = []

    class Probe:
        def __init__(self, emb, precision=None, long_clips=False):
            built.append(long_clips)

    import addvisor_hip.embedder_grad as EG
    monkeypatch.setattr(EG, "EmbedderGrad", Probe)
    monkeypatch.setattr(runtime, "hip_embedder", lambda: None)
    for value, want in ((None, False), ("0", False), ("1", True), ("", False)):
        if value is None:
            monkeypatch.delenv("ADDVISOR_LONG_CLIPS", raising=False)
        else:
            monkeypatch.setenv("ADDVISOR_LONG_CLIPS", value)
        runtime.reset()
        first = runtime.hip_embedder_grad()
        assert runtime.hip_embedder_grad() is first and built[-1] is want, value
    monkeypatch.setenv("ADDVISOR_LONG_CLIPS", "yes")
    runtime.reset()
    with pytest.raises(ValueError, match="ADDVISOR_LONG_CLIPS"):
        runtime.hip_embedder_grad()
    runtime.reset()
