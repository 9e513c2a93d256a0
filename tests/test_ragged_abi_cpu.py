"""CPU-only: the argument contract of the ragged entry points (include/addvisor_hip.h): ADVH_EINVAL / ADVH_EUNSUPPORTED come
back before any HIP call, so they can be exercised without a device.  Also the host-side ``lengths`` validation of
``HipEmbedder`` and the mask / padding helpers of the public interface, none of which needs a GPU."""
import ctypes as C

import pytest
import torch

from addvisor_hip import _lib, synthetic as syn
from addvisor_hip.embedder import HipEmbedder

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    return C.addressof(buf), buf


def test_attention_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_attention_f16_ragged
    assert f(None, p, p, 1, 16, 64, 1, None) == EINVAL and f(p, None, p, 1, 16, 64, 1, None) == EINVAL
    assert f(p, p, None, 1, 16, 64, 1, None) == EINVAL                           # frames NULL
    assert f(p, p, p, 0, 16, 64, 1, None) == EINVAL and f(p, p, p, 1, 0, 64, 1, None) == EINVAL and f(p, p, p, 1, 16, 0, 1, None) == EINVAL
    assert f(p, p, p, 1, 16, 64, 3, None) == EINVAL and f(p, p, p, 1, 16, 64, 0, None) == EINVAL      # H % heads, heads <= 0
    assert f(p, p, p, 1, 257, 64, 1, None) == EUNSUPPORTED                       # T > 256
    assert f(p, p, p, 1, 16, 136, 1, None) == EUNSUPPORTED and f(p, p, p, 1, 16, 20, 1, None) == EUNSUPPORTED     # head dim > 128, % 8
    g = lib.advh_attention_split_ragged
    assert g(None, 8, p, 8, p, 1, 16, 64, 1, None) == EINVAL and g(p, 8, None, 8, p, 1, 16, 64, 1, None) == EINVAL
    assert g(p, 8, p, 8, None, 1, 16, 64, 1, None) == EINVAL
    assert g(p, 8, p, 8, p, 0, 16, 64, 1, None) == EINVAL and g(p, 8, p, 8, p, 1, 0, 64, 1, None) == EINVAL and g(p, 8, p, 8, p, 1, 16, 0, 1, None) == EINVAL
    assert g(p, 8, p, 8, p, 1, 16, 64, 3, None) == EINVAL
    assert g(p, 0, p, 8, p, 1, 16, 64, 1, None) == EINVAL and g(p, 8, p, 0, p, 1, 16, 64, 1, None) == EINVAL      # no lo plane
    assert g(p, 4, p, 8, p, 1, 16, 64, 1, None) == EINVAL and g(p, 8, p, 6, p, 1, 16, 64, 1, None) == EINVAL      # plane distance % 8 / % 4
    assert g(p, 8, p, 8, p, 1, 257, 64, 1, None) == EUNSUPPORTED and g(p, 8, p, 8, p, 1, 16, 136, 1, None) == EUNSUPPORTED
    # the siblings answer the same way
    assert lib.advh_attention_f16(p, p, 1, 257, 64, 1, None) == EUNSUPPORTED and lib.advh_attention_split(p, 4, p, 8, 1, 16, 64, 1, None) == EINVAL


def frontend_args(p, **kw):
    a = dict(wave=p, stride=4000, n_in=4000, B=1, L=4000, w0=p, bias=None, gamma=p, beta=p, mode=0, normalize=1, stats=p, norm=p, mr=None,
             out=p, out_lo=1 << 20, T0=799, P0=800, C0=32, lens=p)
    a.update(kw)
    return a


def call_frontend(lib, split, a):
    head = (a["wave"], a["stride"], a["n_in"], a["B"], a["L"], a["w0"], a["bias"], a["gamma"], a["beta"], a["mode"], a["normalize"],
            a["stats"], a["norm"], a["mr"], a["out"])
    if split:
        return lib.advh_w2v2_frontend_split_ragged(*head, a["out_lo"], a["T0"], a["P0"], a["C0"], a["lens"], None)
    return lib.advh_w2v2_frontend_ragged(*head, a["T0"], a["P0"], a["C0"], a["lens"], None)


@pytest.mark.parametrize("split", [False, True])
def test_frontend_ragged_arguments(lib, p, split):
    p = p[0]
    bad = [dict(lens=None), dict(wave=None), dict(w0=None), dict(stats=None), dict(out=None), dict(B=0), dict(L=9), dict(n_in=0),
           dict(C0=0), dict(C0=12), dict(C0=4096), dict(T0=798), dict(P0=798), dict(stride=100), dict(gamma=None), dict(norm=None),
           dict(mode=2)]
    if split:
        bad += [dict(out_lo=0), dict(out_lo=12)]                                 # a bad plane distance
    for kw in bad:
        assert call_frontend(lib, split, frontend_args(p, **kw)) == EINVAL, kw
    assert call_frontend(lib, split, frontend_args(p, mode=1, gamma=None, beta=None, norm=None, lens=None)) == EINVAL


def test_row_kernels_ragged_arguments(lib, p):
    p = p[0]
    z = lib.advh_zero_tail_rows
    assert z(None, p, 1, 4, 64, None) == EINVAL and z(p, None, 1, 4, 64, None) == EINVAL
    assert z(p, p, 0, 4, 64, None) == EINVAL and z(p, p, 1, 0, 64, None) == EINVAL and z(p, p, 1, 4, 0, None) == EINVAL
    assert z(p, p, 65536, 4, 64, None) == EUNSUPPORTED                           # one grid row per clip
    q = lib.advh_pool_logreg_ragged
    assert q(None, p, 0.0, p, p, None, p, 1, 4, 64, None) == EINVAL and q(p, None, 0.0, p, p, None, p, 1, 4, 64, None) == EINVAL
    assert q(p, p, 0.0, None, p, None, p, 1, 4, 64, None) == EINVAL and q(p, p, 0.0, p, None, None, p, 1, 4, 64, None) == EINVAL
    assert q(p, p, 0.0, p, p, None, None, 1, 4, 64, None) == EINVAL              # frames NULL
    assert q(p, p, 0.0, p, p, None, p, 0, 4, 64, None) == EINVAL and q(p, p, 0.0, p, p, None, p, 1, 0, 64, None) == EINVAL
    assert q(p, p, 0.0, p, p, None, p, 1, 4, 0, None) == EINVAL


def bare_embedder(cfg):
    emb = HipEmbedder.__new__(HipEmbedder)                                       # the host checks need no device
    emb.cfg = cfg
    return emb


def test_lengths_validation_on_the_host():
    emb = bare_embedder(syn.tiny_config(True))
    ok = [4000, 400, 2500]
    assert emb._check_lengths(ok, 3, 4000) == ok
    assert emb._check_lengths(torch.tensor(ok), 3, 4000) == ok and emb._check_lengths(tuple(ok), 3, 4000) == ok
    import numpy as np
    assert emb._check_lengths(np.array(ok), 3, 4000) == ok
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        emb._check_lengths([4000, 400], 3, 4000)
    with pytest.raises(ValueError, match="not an integer"):
        emb._check_lengths([4000, 400.0, 2500], 3, 4000)
    with pytest.raises(ValueError, match="not an integer"):
        emb._check_lengths([4000, True, 2500], 3, 4000)
    with pytest.raises(ValueError, match="integer tensor"):
        emb._check_lengths(torch.tensor([4000.0, 400.0, 2500.0]), 3, 4000)
    with pytest.raises(ValueError, match="integer tensor"):
        emb._check_lengths(torch.tensor([[4000, 400, 2500]]), 3, 4000)
    with pytest.raises(ValueError, match="integer tensor"):
        emb._check_lengths(7, 3, 4000)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 4001 exceeds"):
        emb._check_lengths([4000, 4001, 2500], 3, 4000)
    with pytest.raises(ValueError, match=r"clip 2 has 399 samples.*shortest supported length is 400"):
        emb._check_lengths([4000, 400, 399], 3, 4000)
    with pytest.raises(ValueError, match="clip 0 has -5"):
        emb._check_lengths([-5, 400, 400], 3, 4000)


def test_mask_lengths_and_pad_clips():
    import classifier_embedder as ce
    m = torch.zeros(3, 10, dtype=torch.long)
    m[0, :10], m[1, :4], m[2, :1] = 1, 1, 1
    assert ce.mask_lengths(m, (3, 10)) == [10, 4, 1]
    assert ce.mask_lengths(m.bool(), (3, 10)) == [10, 4, 1] and ce.mask_lengths(m.float(), (3, 10)) == [10, 4, 1]
    holes = m.clone()
    holes[1, 6] = 1
    with pytest.raises(ValueError, match="holes"):
        ce.mask_lengths(holes, (3, 10))
    left = torch.zeros(1, 10, dtype=torch.long)
    left[0, 3:] = 1
    with pytest.raises(ValueError, match="right-padded"):
        ce.mask_lengths(left, (1, 10))
    with pytest.raises(ValueError, match="0 and 1"):
        ce.mask_lengths(m * 2, (3, 10))
    with pytest.raises(ValueError, match="shape"):
        ce.mask_lengths(m, (3, 11))
    import inspect
    assert list(inspect.signature(ce._Wav2Vec2.__call__).parameters)[1:] == ["input_values", "attention_mask", "output_hidden_states"]


def test_pad_clips():
    import inspect

    import audioprocessor
    import captum_saliency
    waves, lengths = audioprocessor.pad_clips([torch.ones(5), torch.full((3,), 2.0), torch.full((7,), 3.0)])
    assert lengths == [5, 3, 7] and waves.shape == (3, 7) and waves.dtype == torch.float32
    assert waves[0].tolist() == [1] * 5 + [0] * 2 and waves[1].tolist() == [2] * 3 + [0] * 4 and waves[2].tolist() == [3.0] * 7
    with pytest.raises(ValueError):
        audioprocessor.pad_clips([])
    with pytest.raises(ValueError):
        audioprocessor.pad_clips([torch.ones(2, 2)])
    for fn in (audioprocessor.AudioProcessor.extract_features, audioprocessor.AudioProcessor.classify, captum_saliency.Wav2vec2LogReg.forward,
               HipEmbedder.forward):
        assert inspect.signature(fn).parameters["lengths"].default is None
