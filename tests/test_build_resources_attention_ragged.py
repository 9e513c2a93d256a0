"""CPU-only: the instances compiled from csrc/attention_ragged.hip are exactly the ones the dispatch mirror of
tests/attention_ragged_cases.py selects for the cases of tests/test_gpu_attention_ragged.py, they are the same classes as the
instances of csrc/attention.hip, and none of them uses scratch or gives up its sibling's occupancy.  Names are read from
hipcc's resource remarks, as tests/test_build_resources_attention.py does."""
import re

import attention_ragged_cases as C
from test_build_resources_backward import instances, resources


def compiled(src, kernels):
    return set().union(*(instances(src, k) for k in kernels))


def test_every_ragged_instance_has_a_case_and_a_sibling():
    ragged = compiled("attention_ragged.hip", C.F16 + C.SPLIT)
    assert len(ragged) == 28, sorted(ragged)
    sel = C.selected()
    assert set(sel) == ragged, (sorted(ragged - set(sel)), sorted(set(sel) - ragged))
    assert {i for i, cs in sel.items() if any(c[0] == "f16" for c in cs)} == compiled("attention_ragged.hip", C.F16)
    assert {i for i, cs in sel.items() if any(c[0] == "split" for c in cs)} == compiled("attention_ragged.hip", C.SPLIT)
    siblings = compiled("attention.hip", tuple(C.SIBLING.values()))
    assert {(C.SIBLING[i[0]],) + i[1:] for i in ragged} == siblings
    for inst, cases in sel.items():                                   # both edges of the tile-count class, by the stride
        if inst[0] == "attention_ragged_x3_stream_kernel":
            assert {c[1] for c in cases} >= set(C.STREAM_STRIDES), inst
            continue
        lo, hi = C.K.CLASSES[inst[1]]
        lo = 16 if lo == 1 else lo                                    # strides start at one whole tile
        if inst == ("attention_ragged_kernel", 13, 128):
            lo = 65                                                   # head dim 128 has no 8-tile instance
        assert {lo, hi} <= {c[1] for c in cases}, (inst, sorted({c[1] for c in cases}))


def test_middle_clip_straddles_an_edge():
    for c in C.CASES:
        T, stream = c[1], c[5]
        full, one, m = C.frames_of(T, stream)
        assert (full, one) == (T, 1) and 1 <= m <= T
        if stream:
            assert abs(m - C.K.STREAM_KB) <= 1 and (m + C.K.STREAM_KB - 1) // C.K.STREAM_KB <= (T + C.K.STREAM_KB - 1) // C.K.STREAM_KB
        else:
            assert m % 16 == 1                                        # one frame into a 16-frame tile


def test_ragged_instances_keep_their_siblings_budget():
    """No scratch, the sibling's occupancy, and at most one VGPR above the sibling (attention_ragged_x3_kernel<13, 64>: 144
    against 143; every other instance has the sibling's count or fewer)."""
    rag, sib = resources("attention_ragged.hip"), resources("attention.hip")

    def by_instance(res, rename):
        out = {}
        for name, v in res.items():
            m = re.search(r"\d+(attention\w*kernel)I((?:L[ib]\d+E)+)E", name)
            if m:
                out[(rename(m.group(1)), m.group(2))] = v
        return out
    rag, sib = by_instance(rag, lambda k: C.SIBLING[k]), by_instance(sib, lambda k: k)
    assert set(rag) == set(sib) and len(rag) == 28
    for k, v in rag.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= sib[k]["occupancy"], (k, v, sib[k])
        assert v["vgprs"] <= sib[k]["vgprs"] + 1, (k, v, sib[k])
