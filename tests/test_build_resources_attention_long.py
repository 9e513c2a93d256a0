"""CPU-only: the instances compiled from csrc/attention_long.hip are exactly the seven the dispatch mirror of
tests/attention_long_cases.py selects for the cases of tests/test_gpu_attention_long.py, every instance is reached at one, two
and three key blocks and at one and several query blocks, none uses scratch, and the inputs of the adversarial cases hold their
preconditions (asserted from the float64 reference, never from a kernel).  Names and figures are read from hipcc's resource
remarks, as tests/test_build_resources_attention.py does."""
import re

import pytest
import torch

import attention_kernel_cases as K
import attention_long_cases as C
from split_contract_ref import split_ref
from test_build_resources_backward import instances, resources

INSTANCES = {(C.KERNEL, 16, 32, 2, False), (C.KERNEL, 16, 64, 2, False), (C.KERNEL, 7, 128, 2, False),
             (C.KERNEL, 16, 32, 1, False), (C.KERNEL, 16, 64, 1, False), (C.KERNEL, 16, 128, 1, False),
             (C.KERNEL, 16, 64, 2, True)}                                # the last: head dim 64 by the LDS DMA
LDS = {(16, 32, 2): 73728, (16, 64, 2): 147456, (7, 128, 2): 147456, (16, 32, 1): 36864, (16, 64, 1): 73728, (16, 128, 1): 147456}
LDS_DMA = 131072                                                         # K and V row-major, two planes of 256 keys x 128 B each


def test_compiled_instances_are_the_seven_and_each_has_its_cases():
    compiled = instances("attention_long.hip", C.KERNEL)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)
    sel = C.selected()
    assert set(sel) == compiled, (sorted(compiled - set(sel)), sorted(set(sel) - compiled))
    for inst, cases in sel.items():
        reach = {C.instance_of(c[0], c[1], c[3])[5:] for c in cases}
        assert {1, 2, 3} <= {kb for kb, _ in reach}, (inst, sorted(reach))              # key blocks
        assert 1 in {qb for _, qb in reach} and max(qb for _, qb in reach) >= 2, (inst, sorted(reach))
        if inst[4]:                                                                     # the DMA instance: head dim 64 and nothing else
            assert {c[3] for c in cases} == {C.DMA_DIM} and all(c[0] == "split" for c in cases)
        else:
            assert any(c[3] < inst[2] and c[2] >= 2 for c in cases), inst               # a padded head dim next to another head
            assert any(c[3] == inst[2] for c in cases) or inst[:4] == (C.KERNEL, 16, 64, 2), inst
        long = {c[1] for c in cases if c[1] > 256}
        assert long >= set(C.T_KB112 if inst[1] == 7 else C.T_KB256), (inst, sorted(long))
    for entry in C.ENTRIES:                                                             # the adversarial inputs reach every instance
        for shapes in (C.UNIFORM_SHAPES, C.PEAKED_SHAPES):
            assert {C.compiled_name(C.instance_of(entry, s[0], s[2])) for s in shapes} == {i for i in INSTANCES if i[3] == (1 if entry == "f16" else 2)}
    assert {C.compiled_name(C.instance_of(c[0], c[1], c[3])) for c in C.ORDERED_CASES} == INSTANCES
    assert {C.compiled_name(C.instance_of(c[0], c[1], c[3])) for c in C.FRAME_CASES} == INSTANCES


def test_key_blocks_fit_the_lds_budget():
    """K [KB][D] + V^T [D][KB + 64] in NP planes of fp16: the figures of the instance table, all within 160 KiB."""
    for (ntb, D, np_), want in LDS.items():
        kb = ntb * 16
        assert np_ * (kb * D + D * (kb + 64)) * 2 == want <= 160 * 1024
    assert 2 * 2 * 256 * 64 * 2 == LDS_DMA <= 160 * 1024


def test_long_instances_do_not_spill():
    """No scratch in any instance (attention_x3_stream_kernel<7, 128>, whose loop <7, 128, 2> is, has none either), and at least
    two wavefronts per SIMD: the workgroup is eight wavefronts on four SIMDs."""
    res = {k: v for k, v in resources("attention_long.hip").items() if re.search(rf"\d+{C.KERNEL}I", k)}
    assert len(res) == 7, sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)
        assert v["vgprs"] <= 256, (k, v)


def test_frames_cases_hold_what_the_gpu_test_relies_on():
    for T, sets in C.FRAMES.items():
        assert [s[:2] for s in sets] == [(T, 1), (T, 256), (T, 17)] and [s[2] for s in sets][:2] == [257, 273]
        assert all(s[2] % 16 == 1 and 1 <= s[2] <= T for s in sets) and sets[2][2] <= 256
    for c in C.FRAME_CASES:
        assert c[1] in C.FRAMES and c[4] == 3


@pytest.mark.parametrize("case", C.ORDERED_CASES, ids=C.case_id)
def test_ordered_maxima_sit_in_their_blocks(case):
    """Three key blocks of the instance's own size; the row maximum of query i lies in block i % 3, the best score of each other
    block at least 40 below it; for target 2 the running maximum rises twice; q and k are multiples of 1/8."""
    entry, T, heads, dm, B = case
    KB = C.key_block(entry, dm)
    ref = C.reference("ordered", entry, T, heads, dm, B)
    assert C.instance_of(entry, T, dm)[5] == 3
    for t in (ref["q"], ref["k"]):
        assert torch.equal(t * 8.0, torch.round(t * 8.0))
    s = K.scores(ref)
    blk, tgt = C.ordered_block(T, KB), K.ordered_target(T)
    assert sorted(set(blk.tolist())) == [0, 1, 2] and all((tgt == c).sum().item() >= T // 3 for c in range(3))
    best = torch.stack([s[..., blk == c].max(-1).values for c in range(3)], -1)
    assert torch.equal(best.argmax(-1), tgt.expand(B, heads, T))
    own = best.gather(-1, tgt.expand(B, heads, T).unsqueeze(-1))
    others = best.masked_fill(torch.nn.functional.one_hot(tgt, 3).bool().expand_as(best), float("-inf"))
    margin = (own - others.max(-1, keepdim=True).values).min().item()
    print(f"ordered {C.case_id(case)}: smallest margin {margin:.2f}, max|score| {s.abs().max().item():.2f}")
    assert margin >= K.ORDERED_GAP
    rise = best[..., tgt == 2, :]
    assert (rise[..., 0] < rise[..., 1]).all() and (rise[..., 1] < rise[..., 2]).all()
    assert s.abs().max().item() < 30.0


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.UNIFORM_SHAPES, ids=str)
def test_uniform_probabilities_are_one_over_t(entry, shape):
    ref = C.reference("uniform", entry, *shape)
    assert not ref["q"].any()
    assert (ref["p"] - 1.0 / shape[0]).abs().max().item() <= 2.0 ** -53
    assert (ref["ctx"] - ref["v"].mean(-2, keepdim=True)).abs().max().item() <= 1e-14


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.PEAKED_SHAPES, ids=str)
def test_peaked_rows_are_peaked(entry, shape):
    ref = C.reference("peaked", entry, *shape)
    s = K.scores(ref)
    top = ref["p"].max(-1)
    assert top.values.min().item() > 0.999
    assert torch.equal(top.indices, torch.arange(shape[0]).expand_as(top.indices))
    assert (s.max(-1).values - s.min(-1).values).min().item() > K.PEAK_SPAN
    assert s.abs().max().item() < K.PEAK_SCORE * 1.01


@pytest.mark.parametrize("s", [x for x in C.all_input_sets() if x[0] != "random" or x[2] > 256], ids=K.set_id)
def test_bars_are_within_reach_of_fp32(s):
    """As tests/test_attention_kernel_cases_cpu.py: a plain numpy fp32 restatement stays within half the split bar on these
    inputs, and the split rounding of the fp64 result within a tenth of it."""
    kind, entry, T, heads, dm, B = s
    ref = C.reference(kind, entry, T, heads, dm, B)
    np32 = K.split_ratio(K.attention_np32(ref["q"], ref["k"], ref["v"]), ref["ctx"])
    print(f"{K.set_id(s)}: numpy fp32 |err| / split bar {np32:.3f}")
    assert np32 <= 0.5, np32
    if entry == "split":
        hi, lo, over = split_ref(ref["ctx"])
        assert not over.any()
        assert K.split_ratio(hi.double() + lo.double() / 2048.0, ref["ctx"]) <= 0.1
