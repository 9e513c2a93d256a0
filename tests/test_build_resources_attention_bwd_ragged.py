"""CPU-only: the ragged attention-backward instances -- the RAGGED = true instantiations of attention_bwd_kernel (backward.hip),
attention_bwd_x3_kernel (attention_bwd_x3.hip) and attention_bwd_f32_kernel (attention_bwd_f32.hip) -- are the siblings' set (the
same template arguments with RAGGED = false), each is selected by a case of tests/test_gpu_attention_bwd_ragged.py at both edges
of its tile-count class, and each keeps its sibling's budget.  Names and figures are read from hipcc's resource remarks, as
tests/test_build_resources_backward.py does."""
import re

import attention_bwd_ragged_cases as C
from test_build_resources_backward import instances, resources


def test_every_ragged_instance_has_a_case_and_a_sibling():
    compiled = set().union(*(instances(src, k) for k, src in C.SOURCES.items()))
    ragged, siblings = {i for i in compiled if i[-1]}, {i for i in compiled if not i[-1]}
    assert len(ragged) == 15 + 8 + 12 and len(siblings) == 15 + 8 + 12, sorted(compiled)
    assert {C.sibling(i) for i in ragged} == siblings
    sel = C.selected()
    refused = {C.instance_of("f16", T, dm) for T, dm in C.REFUSED}
    assert refused == {("attention_bwd_kernel", 16, 128, False, True)}       # compiled, above 160 KiB of LDS: never launched, as the sibling
    assert not refused & set(sel)
    assert set(sel) | refused == ragged, (sorted(ragged - set(sel) - refused), sorted(set(sel) - ragged))
    for inst, cases in sel.items():                                          # both edges of the tile-count class, by the stride
        lo, hi = C.CLASSES[inst[1]]
        if inst[0] == "attention_bwd_kernel" and inst[2] == 128 and inst[1] == 13:
            lo = 65                                                          # head dim 128 has no 8-tile instance
        assert {lo, hi} <= {c[1] for c in cases}, (inst, sorted({c[1] for c in cases}))
        assert all(c[2] >= 2 and c[4] == 3 for c in cases)                   # two heads, three clips


def test_middle_clip_is_one_frame_into_a_tile():
    for T in C.STRIDES:
        full, one, m = C.frames_of(T)
        assert (full, one) == (T, 1) and 1 <= m <= T and m % 16 == 1


def test_ragged_instances_keep_their_siblings_budget():
    """The sibling's occupancy, no more scratch than the sibling (attention_bwd_x3_kernel<13, 64, 8> keeps 68 bytes, every other
    instance none) and at most one VGPR above the sibling -- the slack the forward's ragged kernels were allowed; measured: every
    instance has the sibling's count, attention_bwd_x3_kernel<13, 32, 8, true> two fewer.  LDS is dynamic and sized by the
    launcher both instances share (same template arguments, same bytes)."""
    rag, sib = {}, {}
    for src in C.SOURCES.values():
        for name, v in resources(src).items():
            m = re.search(r"\d+(attention_bwd\w*kernel)I((?:L[ib]\d+E)+)Lb([01])EE", name)
            if m:
                (rag if m.group(3) == "1" else sib)[(m.group(1), m.group(2))] = v
    assert set(rag) == set(sib) and len(rag) == 35
    for k, v in rag.items():
        print(k, v, sib[k])
        assert v["scratch"] <= sib[k]["scratch"], (k, v, sib[k])
        assert v["occupancy"] >= sib[k]["occupancy"], (k, v, sib[k])
        assert v["vgprs"] <= sib[k]["vgprs"] + 1, (k, v, sib[k])
    assert sib[("attention_bwd_x3_kernel", "Li13ELi64ELi8E")]["scratch"] == 68
    assert sum(v["scratch"] for v in sib.values()) == 68
