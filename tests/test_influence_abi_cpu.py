"""CPU-only: the error contract of the entry points of csrc/influence.hip (ADVH_EINVAL before any HIP call, so it can be
exercised without a GPU) and the sizes the three ``_workspace`` functions return, against their rules restated here."""
import ctypes as C

import pytest

from addvisor_hip import _lib, influence as INF

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


def refuses(f, ok, nulls, bad):
    for i in nulls:
        args = list(ok)
        args[i] = None
        assert f(*args) == EINVAL, i
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert f(*args) == EINVAL, (i, v)


def test_moment_argument_errors(lib, p):
    ok = [p, 8, p, 4, 8, p, p, None]                                         # X, ldx, w, N, F, workspace, Hm, stream
    refuses(lib.advh_influence_moment, ok, (0, 5, 6),
            ((1, 7), (3, 0), (3, -1), (3, (1 << 24) + 1), (4, 0), (4, -2), (4, 4097), (0, p + 2), (2, p + 1), (5, p + 2), (6, p + 4)))
    for bad in ((0, 1), (1, 0), (-1, 1), ((1 << 24) + 1, 1), (1, 4097)):
        assert lib.advh_influence_moment_workspace(*bad) == EINVAL
        with pytest.raises(_lib.AdvhError):
            INF.moment_workspace(*bad)


def test_sqdist_and_sumsq_argument_errors(lib, p):
    ok = [p, 8, p, 8, 2, 2, 8, p, p, None]                                   # X, ldx, Y, ldy, M, N, F, workspace, D, stream
    refuses(lib.advh_influence_sqdist, ok, (0, 2, 7, 8),
            ((1, 7), (3, 7), (4, 0), (5, 0), (6, 0), (4, -1), (6, -3), (4, (1 << 20) + 1), (5, (1 << 20) + 1), (0, p + 2), (2, p + 1),
             (7, p + 2), (8, p + 4)))
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), ((1 << 20) + 1, 1, 1)):
        assert lib.advh_influence_sqdist_workspace(*bad) == EINVAL
        with pytest.raises(_lib.AdvhError):
            INF.sqdist_workspace(*bad)
    ok = [p, 8, 2, 8, p, None]                                               # X, ldx, M, F, out, stream
    refuses(lib.advh_influence_sumsq, ok, (0, 4), ((1, 7), (2, 0), (2, -1), (2, (1 << 24) + 1), (3, 0), (3, -1), (0, p + 1), (4, p + 4)))


def test_elementwise_argument_errors(lib, p):
    ok = [p, p, 4, 2, p, None]                                               # Z, y, N, C, out, stream
    refuses(lib.advh_influence_residual, ok, (0, 1, 4), ((2, 0), (2, -1), (2, (1 << 24) + 1), (3, 0), (3, 65537), (0, p + 4), (1, p + 2), (4, p + 1)))
    ok = [p, p, p, 2, 4, p, 4, None]                                         # G, a, b, M, N, out, ldo, stream
    refuses(lib.advh_influence_cosine, ok, (0, 1, 2, 5),
            ((3, 0), (3, (1 << 20) + 1), (4, 0), (4, (1 << 24) + 1), (6, 3), (0, p + 4), (1, p + 4), (2, p + 4), (5, p + 2)))
    ok = [p, 2, 4, p, 4, None]                                               # D, M, N, out, ldo, stream
    refuses(lib.advh_influence_root, ok, (0, 3), ((1, 0), (1, -1), (2, 0), (2, (1 << 24) + 1), (4, 3), (0, p + 4), (3, p + 1)))
    ok = [p, p, p, p, 3, 2, 4, p, 4, None]                                   # G, rt, rn, lr, C, M, N, out, ldo, stream
    refuses(lib.advh_influence_scale, ok, (0, 1, 2, 3, 7),
            ((4, 0), (4, 65537), (5, 0), (5, (1 << 20) + 1), (6, 0), (6, (1 << 24) + 1), (8, 3), (0, p + 4), (3, p + 4), (1, p + 2), (2, p + 1),
             (7, p + 2)))
    ok = [p, p, p, 3, 4, p, None]                                            # ss, rn, lr, C, N, out, stream
    refuses(lib.advh_influence_self_scale, ok, (0, 1, 2, 5),
            ((3, 0), (3, 65537), (4, 0), (4, (1 << 24) + 1), (0, p + 4), (2, p + 4), (1, p + 2), (5, p + 1)))


def test_topk_argument_errors(lib, p):
    ok = [p, 8, 2, 8, 3, 1, p, p, p, None]                                   # S, lds, M, N, k, largest, workspace, idx, val, stream
    refuses(lib.advh_influence_topk, ok, (0, 6, 7, 8),
            ((1, 7), (2, 0), (2, 65536), (3, 0), (3, (1 << 24) + 1), (4, 0), (4, 9), (4, -1), (5, 2), (5, -1), (0, p + 2), (6, p + 4),
             (7, p + 2), (8, p + 1)))
    assert lib.advh_influence_topk(p, 1000, 1, 1000, 257, 1, p, p, p, None) == EINVAL    # k > 256
    for bad in ((0, 8, 1), (1, 0, 1), (1, 8, 0), (1, 8, 9), (1, 1000, 257), (65536, 8, 1), (1, (1 << 24) + 1, 1)):
        assert lib.advh_influence_topk_workspace(*bad) == EINVAL
        with pytest.raises(_lib.AdvhError):
            INF.topk_workspace(*bad)


def moment_slab(N, F):
    """The slab length of include/addvisor_hip.h, restated."""
    b = -(-F // 64)
    per = -(-N // max(1, 1024 // (b * (b + 1) // 2)))
    return max(512, -(-per // 32) * 32)


@pytest.mark.parametrize("N,F", [(1, 1), (3, 5), (70, 65), (130, 129), (1100, 193), (3136, 70), (4099, 33), (65536, 769), (40, 65),
                                 (1 << 24, 4096), (100000, 1921)])
def test_moment_workspace_sizes(lib, N, F):
    S = moment_slab(N, F)
    assert S % 32 == 0
    assert lib.advh_influence_moment_workspace(N, F) == INF.moment_workspace(N, F) == -(-N // S) * F * F * 4


def test_moment_workspace_facts(lib):
    assert moment_slab(1100, 193) == 512 and INF.moment_workspace(1100, 193) == 3 * 193 * 193 * 4     # two full slabs plus 76 rows
    assert moment_slab(65536, 769) == 5984 and -(-65536 // 5984) == 11                                # 91 blocks x 11 slabs
    # a 1921 x 1921 problem gives 496 workgroups per slab, and long indexes two slabs of them
    assert 31 * 32 // 2 == 496 and moment_slab(100000, 1921) == 50016 and INF.moment_workspace(100000, 1921) == 2 * 1921 * 1921 * 4


def gram_slab(M, N, F):
    blocks = -(-M // 64) * -(-N // 64)
    per = -(-F // max(1, 1024 // blocks))
    return max(512, -(-per // 64) * 64)


@pytest.mark.parametrize("M,N,F", [(1, 1, 1), (5, 3, 1000), (3, 4, 1029), (70, 65, 130), (33, 33, 4099), (16, 1024, 152832), (6, 40, 3136)])
def test_sqdist_workspace_sizes(lib, M, N, F):
    S = gram_slab(M, N, F)
    assert lib.advh_influence_sqdist_workspace(M, N, F) == INF.sqdist_workspace(M, N, F) == -(-F // S) * M * N * 4
    assert lib.advh_influence_sqdist_workspace(M, N, F) == lib.advh_concept_gram_workspace(M, N, F)   # the Gram kernel's plan


def topk_bytes(M, N, k):
    c1 = -(-N // 2048)
    c2 = -(-c1 * k // 2048)
    return max(16, 8 * M * k * ((c1 if c1 > 1 else 0) + (c2 if c1 > 1 and c2 > 1 else 0)))


@pytest.mark.parametrize("M,N,k", [(1, 1, 1), (3, 7, 7), (2, 1000, 5), (5, 4099, 64), (2, 70000, 256), (16, 65536, 10), (1, 1 << 24, 256),
                                   (4, 2048, 256), (4, 2049, 256)])
def test_topk_workspace_sizes(lib, M, N, k):
    assert lib.advh_influence_topk_workspace(M, N, k) == INF.topk_workspace(M, N, k) == topk_bytes(M, N, k)


def test_topk_workspace_facts(lib):
    assert INF.topk_workspace(4, 2048, 256) == 16                            # one chunk: no keys are kept
    assert INF.topk_workspace(5, 4099, 64) == 8 * 5 * 64 * 3                 # three chunks, whose 192 keys are one chunk
    assert INF.topk_workspace(2, 70000, 256) == 8 * 2 * 256 * (35 + 5)       # 35 chunks keep 8960 keys: five chunks more
