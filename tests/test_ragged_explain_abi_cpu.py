"""CPU-only: the four entry points of the ragged explanation pipeline (csrc/stft_ragged.hip, csrc/unet_ragged.hip) are declared in
include/addvisor_hip.h, bound in ``_lib.SIGNATURES`` and exported, and their argument errors come back as negative codes before
any HIP call, so they can be exercised without a device.  Every call here is malformed on purpose: a well-formed one would launch
on a machine where another test has initialised the library."""
import ctypes as C
import os
import re

import pytest

from addvisor_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("advh_stft_forward_ragged", "advh_istft_masked_c64_ragged", "advh_fmap_clip_tail", "advh_zero_tail_cols_f32")
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 4096)()
    a = C.addressof(buf)
    assert a % 16 == 0
    return a, buf


def test_header_bindings_and_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "addvisor_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(rf"\bint {name}\s*\(([^)]*)\)", text)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), name
        for a, ct in zip(params, args):                                      # pointer / int64 / int by position
            want = C.c_void_p if "*" in a or a.startswith("advh_stream_t") else C.c_int64 if a.startswith("int64_t") else C.c_int
            assert ct is want, (name, a)
        assert hasattr(lib, name), name
    for src in ("stft_ragged.hip", "unet_ragged.hip"):
        assert os.path.exists(os.path.join(ROOT, "xai-audio-deepfakes_amd", "csrc", src))


def stft_args(p, **kw):
    a = dict(wave=p, stride=8000, lens=p, B=2, L=8000, hop=322, win=644, window=None, X=p, mag=p, phase=p, T=25)
    a.update(kw)
    return [a[k] for k in ("wave", "stride", "lens", "B", "L", "hop", "win", "window", "X", "mag", "phase", "T")] + [None]


def test_stft_forward_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_stft_forward_ragged
    bad = [dict(wave=None), dict(lens=None), dict(B=0), dict(L=0), dict(L=512, T=2), dict(hop=0), dict(win=0), dict(win=1026), dict(win=643),
           dict(T=24), dict(stride=7999), dict(X=None, mag=None, phase=None), dict(wave=p + 2), dict(lens=p + 1), dict(X=p + 4),
           dict(mag=p + 2), dict(phase=p + 1), dict(window=p + 3)]
    for kw in bad:
        assert f(*stft_args(p, **kw)) == EINVAL, kw
    assert f(*stft_args(p, B=65536)) == EUNSUPPORTED


def istft_args(p, **kw):
    a = dict(spec=p, mask=p, Fm=512, Tm=24, mode=2, w_in=p, w_out=p, stride=8000, lens=p, B=2, T=25, L=8000, hop=322, win=644, window=None)
    a.update(kw)
    return [a[k] for k in ("spec", "mask", "Fm", "Tm", "mode", "w_in", "w_out", "stride", "lens", "B", "T", "L", "hop", "win", "window")] + [None]


def test_istft_masked_c64_ragged_arguments(lib, p):
    p = p[0]
    f = lib.advh_istft_masked_c64_ragged
    bad = [dict(spec=None), dict(mask=None), dict(lens=None), dict(w_in=None, w_out=None), dict(Fm=0), dict(Fm=514), dict(Tm=0), dict(Tm=26),
           dict(mode=0), dict(mode=3), dict(stride=7999), dict(B=0), dict(T=26), dict(L=512, T=2), dict(hop=0), dict(win=646 - 1),
           dict(spec=p + 4), dict(mask=p + 2), dict(w_in=p + 1), dict(w_out=p + 3), dict(lens=p + 2), dict(window=p + 1)]
    for kw in bad:
        assert f(*istft_args(p, **kw)) == EINVAL, kw
    assert f(*istft_args(p, B=65536)) == EUNSUPPORTED
    assert f(*istft_args(p, hop=128, win=1024, T=63)) == EUNSUPPORTED            # eight overlapping frames at 8 frames per workgroup


def tail_args(p, **kw):
    a = dict(x=p, lo=0, widths=p, shift=0, B=2, H=8, W=24, C=32, PH=1, PW=1, ind=-1)
    a.update(kw)
    return [a[k] for k in ("x", "lo", "widths", "shift", "B", "H", "W", "C", "PH", "PW", "ind")] + [None]


def test_fmap_clip_tail_arguments(lib, p):
    p = p[0]
    f = lib.advh_fmap_clip_tail
    plane = 2 * 10 * 26 * 32
    bad = [dict(x=None), dict(widths=None), dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(C=12), dict(PH=-1), dict(PW=-1), dict(shift=-1),
           dict(shift=3), dict(x=p + 8), dict(widths=p + 2), dict(lo=-8), dict(lo=plane + 4), dict(lo=plane - 8), dict(ind=32)]
    for kw in bad:
        assert f(*tail_args(p, **kw)) == EINVAL, kw
    assert f(*tail_args(p, B=65536)) == EUNSUPPORTED and f(*tail_args(p, H=65536)) == EUNSUPPORTED


def test_zero_tail_cols_f32_arguments(lib, p):
    p = p[0]
    f = lib.advh_zero_tail_cols_f32
    for args in ((None, p, 2, 8, 24), (p, None, 2, 8, 24), (p, p, 0, 8, 24), (p, p, 2, 0, 24), (p, p, 2, 8, 0), (p + 2, p, 2, 8, 24),
                 (p, p + 1, 2, 8, 24)):
        assert f(*args, None) == EINVAL, args
    assert f(p, p, 65536, 8, 24, None) == EUNSUPPORTED
