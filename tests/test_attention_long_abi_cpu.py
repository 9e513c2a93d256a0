"""CPU-only: the argument contract of advh_attention_long_f16 / advh_attention_long_split (include/addvisor_hip.h).  ADVH_EINVAL
and ADVH_EUNSUPPORTED come back before any HIP call, so they can be exercised without a device.  Also: the four whole-clip entry
points keep refusing T > 256, and the gradient chain names its limit on the host before it allocates or launches anything."""
import ctypes as C

import pytest
import torch

from addvisor_hip import _lib, synthetic as syn
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import EmbedderGrad, check_chain_frames

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    return C.addressof(buf), buf


def test_attention_long_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_long_f16
    assert f(None, p, p, 1, 300, 64, 1, None) == EINVAL and f(p, None, p, 1, 300, 64, 1, None) == EINVAL
    assert f(p, p, p, 0, 300, 64, 1, None) == EINVAL and f(p, p, p, 1, 0, 64, 1, None) == EINVAL and f(p, p, p, 1, 300, 0, 1, None) == EINVAL
    assert f(p, p, p, -1, 300, 64, 1, None) == EINVAL and f(p, p, p, 1, -5, 64, 1, None) == EINVAL
    assert f(p, p, p, 1, 300, 64, 3, None) == EINVAL and f(p, p, p, 1, 300, 64, 0, None) == EINVAL      # H % heads, heads <= 0
    assert f(p, p, p, 1, 300, 136, 1, None) == EUNSUPPORTED and f(p, p, p, 1, 300, 20, 1, None) == EUNSUPPORTED   # head dim > 128, % 8
    assert f(p, p, p, 65536, 300, 64, 1, None) == EUNSUPPORTED                    # one grid row per clip
    assert f(p, p, p, 1, 65535 * 128 + 1, 64, 1, None) == EUNSUPPORTED            # 65 536 query blocks
    assert f(p, p, None, 65536, 300, 64, 1, None) == EUNSUPPORTED                 # frames may be NULL: no EINVAL for it
    g = lib.advh_attention_long_split
    assert g(None, 8, p, 8, p, 1, 300, 64, 1, None) == EINVAL and g(p, 8, None, 8, p, 1, 300, 64, 1, None) == EINVAL
    assert g(p, 8, p, 8, p, 0, 300, 64, 1, None) == EINVAL and g(p, 8, p, 8, p, 1, 0, 64, 1, None) == EINVAL and g(p, 8, p, 8, p, 1, 300, 0, 1, None) == EINVAL
    assert g(p, 8, p, 8, p, 1, 300, 64, 3, None) == EINVAL and g(p, 8, p, 8, p, 1, 300, 64, 0, None) == EINVAL
    assert g(p, 0, p, 8, p, 1, 300, 64, 1, None) == EINVAL and g(p, 8, p, 0, p, 1, 300, 64, 1, None) == EINVAL      # no lo plane
    assert g(p, 4, p, 8, p, 1, 300, 64, 1, None) == EINVAL and g(p, 8, p, 6, p, 1, 300, 64, 1, None) == EINVAL      # plane distance % 8 / % 4
    assert g(p, 8, p, 8, p, 1, 300, 136, 1, None) == EUNSUPPORTED and g(p, 8, p, 8, p, 1, 300, 20, 1, None) == EUNSUPPORTED
    assert g(p, 8, p, 8, p, 65536, 300, 64, 1, None) == EUNSUPPORTED and g(p, 8, p, 8, None, 1, 65535 * 128 + 1, 64, 1, None) == EUNSUPPORTED
    assert g(p, 4, p, 8, None, 65536, 300, 64, 1, None) == EINVAL                 # an argument error comes first


def test_whole_clip_entries_keep_their_limit(lib, p):
    p = p[0]
    assert lib.advh_attention_f16(p, p, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_split(p, 8, p, 8, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_f16_ragged(p, p, p, 1, 257, 64, 1, None) == EUNSUPPORTED
    assert lib.advh_attention_split_ragged(p, 8, p, 8, p, 1, 257, 64, 1, None) == EUNSUPPORTED


def bare_embedder(cfg):
    emb = HipEmbedder.__new__(HipEmbedder)                                        # the host checks need no device
    emb.cfg = cfg
    return emb


def test_sample_limit_follows_the_feature_encoder():
    emb = bare_embedder(syn.tiny_config(False))
    assert HipEmbedder.WHOLE_CLIP_MAX_FRAMES == 256
    assert emb.whole_clip_max_samples() == 82319
    assert emb._lengths(82319)[-1] == 256 and emb._lengths(82320)[-1] == 257
    assert emb._lengths(96000)[-1] == 299 and emb._lengths(164240)[-1] == 513 and emb._lengths(160000)[-1] == 499


def test_gradient_chain_names_its_limit_before_any_launch():
    """EmbedderGrad.forward raises on the host: a bare chain with no workspace, no library handle and a CPU tensor gets as far as
    the check and no further."""
    emb = bare_embedder(syn.tiny_config(False))
    check_chain_frames(emb, 82319)
    eg = EmbedderGrad.__new__(EmbedderGrad)
    eg.emb, eg.cfg, eg.split = emb, emb.cfg, False
    for kw in (dict(), dict(lengths=[96000, 50000])):
        with pytest.raises(_lib.AdvhError, match=r"256 frames \(82319 samples\).*T = 299 \(96000 samples\).*forward-only") as e:
            eg.forward(torch.zeros(2, 96000), **kw)
        assert "ADVH_EUNSUPPORTED" in str(e.value)
    with pytest.raises(_lib.AdvhError, match="T = 257"):
        eg.forward(torch.zeros(1, 100000), length=82320)
