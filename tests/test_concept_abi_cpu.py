"""CPU-only: the error contract of the entry points of csrc/concept.hip (ADVH_EINVAL before any HIP call, so it can be exercised
without a GPU) and the sizes ``advh_concept_gram_workspace`` returns."""
import ctypes as C

import pytest

from addvisor_hip import _lib, concept as CO

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_double * 256)()                                               # 8-byte aligned; + 4 is 4-byte aligned only
    a = C.addressof(buf)
    yield a + (-a % 16)
    del buf


def test_gram_argument_errors(lib, p):
    f = lib.advh_concept_gram
    ok = [p, 8, p, 8, 2, 2, 8, 0, p, p, None]                                # X, ldx, Y, ldy, M, N, F, symmetric, workspace, G, stream
    for i in (0, 2, 8, 9):
        args = list(ok)
        args[i] = None
        assert f(*args) == EINVAL, i
    for i, v in ((1, 7), (3, 7), (4, 0), (5, 0), (6, 0), (4, -1), (6, -3), (7, 2), (7, -1), (4, (1 << 20) + 1), (0, p + 2), (2, p + 1),
                 (8, p + 2), (9, p + 4)):
        args = list(ok)
        args[i] = v
        assert f(*args) == EINVAL, (i, v)
    sym = [p, 8, p, 8, 2, 2, 8, 1, p, p, None]
    for i, v in ((2, p + 16), (5, 3), (3, 12)):                              # symmetric: Y == X, M == N, ldy == ldx
        args = list(sym)
        args[i] = v
        assert f(*args) == EINVAL, (i, v)


def test_combine_and_time_pool_argument_errors(lib, p):
    f = lib.advh_concept_combine
    ok = [p, p, 8, 2, 3, 8, p, 8, None]                                      # A, X, ldx, C, N, F, W, ldw, stream
    for i in (0, 1, 6):
        args = list(ok)
        args[i] = None
        assert f(*args) == EINVAL, i
    for i, v in ((2, 7), (7, 7), (3, 0), (4, 0), (5, 0), (3, -2), (0, p + 2), (1, p + 1), (6, p + 3)):
        args = list(ok)
        args[i] = v
        assert f(*args) == EINVAL, (i, v)
    g = lib.advh_concept_time_pool
    ok = [p, 2, 3, 4, 0, p, None]                                            # X, R, T, H, mode, out, stream
    for i in (0, 5):
        args = list(ok)
        args[i] = None
        assert g(*args) == EINVAL, i
    for i, v in ((1, 0), (2, 0), (3, 0), (1, -1), (4, 2), (4, -1)):
        args = list(ok)
        args[i] = v
        assert g(*args) == EINVAL, (i, v)


def slab(M, N, F):
    """The slab length of include/addvisor_hip.h, restated."""
    blocks = -(-M // 64) * -(-N // 64)
    per = -(-F // max(1, 1024 // blocks))
    return max(512, -(-per // 64) * 64)


@pytest.mark.parametrize("M,N,F", [(1, 1, 1), (2, 2, 7), (5, 3, 1000), (33, 33, 4099), (70, 70, 3136), (8, 6, 3136), (3, 3, 1029),
                                   (128, 128, 152832), (16, 8, 152832), (3184, 8, 768), (200, 200, 152832), (1000, 1000, 100)])
def test_gram_workspace_sizes(lib, M, N, F):
    S = slab(M, N, F)
    assert S % 64 == 0
    assert lib.advh_concept_gram_workspace(M, N, F) == CO.gram_workspace(M, N, F) == -(-F // S) * M * N * 4


def test_gram_workspace_facts(lib):
    assert slab(3, 3, 1029) == 512 and CO.gram_workspace(3, 3, 1029) == 3 * 9 * 4        # two full slabs plus 5
    assert CO.gram_workspace(128, 128, 152832) == 239 * 128 * 128 * 4                    # 2 x 64 clips, wav2vec2-base at 4 s
    # a 200 x 200 problem still fills the chip: 16 blocks (10 in symmetric mode) x 63 slabs
    assert slab(200, 200, 152832) == 2432 and -(-152832 // 2432) == 63
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), ((1 << 20) + 1, 1, 1)):
        assert lib.advh_concept_gram_workspace(*bad) == EINVAL
        with pytest.raises(_lib.AdvhError):
            CO.gram_workspace(*bad)
