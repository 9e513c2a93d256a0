"""CPU-only: the instances compiled from csrc/attention_bwd_long.hip are exactly the six the dispatch mirror of
tests/attention_bwd_long_cases.py selects for the cases of tests/test_gpu_attention_bwd_long.py (two kernels x three padded head
dims; the operand format is a run-time argument), every instance is reached at one, two and three or more blocks of its streaming
loop and at one and several workgroups per (clip, head), none uses scratch, the LDS formula of DESIGN 4.34 stays within 160 KiB,
and the inputs of the adversarial cases hold their preconditions (asserted from the float64 reference, never from a kernel).  Names
and figures are read from hipcc's resource remarks, as tests/test_build_resources_attention_long.py does."""
import re

import pytest
import torch

import attention_bwd_long_cases as C
import attention_kernel_cases as AK
import attention_long_cases as AL
from split_contract_ref import split_ref
from test_build_resources_backward import instances, resources

SRC = "attention_bwd_long.hip"
INSTANCES = {(k, D) for k in (C.QUERY_KERNEL, C.KEY_KERNEL) for D in (32, 64, 128)}
LDS = {(C.QUERY_KERNEL, 32): 36864, (C.QUERY_KERNEL, 64): 69632, (C.QUERY_KERNEL, 128): 135168,
       (C.KEY_KERNEL, 32): 38400, (C.KEY_KERNEL, 64): 71168, (C.KEY_KERNEL, 128): 136704}      # the instance table of DESIGN 4.34


def test_compiled_instances_are_the_six_and_each_has_its_cases():
    compiled = instances(SRC, C.QUERY_KERNEL) | instances(SRC, C.KEY_KERNEL)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)
    sel = C.selected()
    assert set(sel) == compiled, (sorted(compiled - set(sel)), sorted(set(sel) - compiled))
    for inst, hits in sel.items():
        loops, wgs = {l for _, l, _ in hits}, {w for _, _, w in hits}
        assert {1, 2, 3} <= loops and max(loops) >= 4, (inst, sorted(loops))             # blocks of the streaming loop
        assert 1 in wgs and max(wgs) >= 2, (inst, sorted(wgs))                           # workgroups per (clip, head)
        cases = [c for c, _, _ in hits]
        assert {c[0] for c in cases} == set(C.ENTRIES), inst                             # both formats run every instance
        assert any(c[3] < inst[1] and c[2] >= 2 for c in cases), inst                    # a padded head dim next to another head
        assert any(c[3] == inst[1] for c in cases), inst                                 # and the exact one
        assert {c[1] for c in cases} >= set(C.T_ALL), inst
    for b in C.BLOCKS:                                                                   # the strides the issue asks for per block size
        assert {b, b + 1, 2 * b, 2 * b + 1, 2 * b + 17, 3 * b + 1} <= set(C.T_ALL)
    assert {1, 16, 17, 256, 257, 513} <= set(C.T_ALL)
    for shapes in (C.KIND_SHAPES, [c[1:] for c in C.FRAME_CASES]):                       # adversarial inputs and frames reach all six
        assert {(k, D) for s in shapes for k, D, _, _ in C.instances_of("split", s[0], s[2])} == INSTANCES
    assert all(s[0] == C.ADVERSARIAL_T == 2 * C.KB + 17 for s in C.KIND_SHAPES)


def test_block_sizes_fit_the_lds_budget():
    """Two fp32 matrices [block][D + 4], and three floats per staged query in the key kernel: the figures of the instance table."""
    for (kernel, D), want in LDS.items():
        got = C.lds_query(D) if kernel == C.QUERY_KERNEL else C.lds_key(D)
        assert got == want <= 160 * 1024, (kernel, D, got)
    assert C.lds_query(128) == 2 * C.KB * 132 * 4 and C.lds_key(128) == (2 * C.SQB * 132 + 3 * C.SQB) * 4
    assert C.QB == C.KWB == 128 and C.QB % 16 == 0 and C.KB % 16 == 0 and C.SQB % 16 == 0     # eight wavefronts, one tile each


def test_long_backward_instances_do_not_spill():
    """No scratch in any instance, and at least two wavefronts per SIMD (the workgroup is eight wavefronts on four SIMDs): the
    fp32-input MFMA has a 40-cycle dependent latency on a 32-cycle issue."""
    res = {k: v for k, v in resources(SRC).items() if re.search(rf"\d+({C.QUERY_KERNEL}|{C.KEY_KERNEL})I", k)}
    assert len(res) == 6, sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)
        assert v["vgprs"] <= 256, (k, v)


def test_workspace_and_frames_cases():
    assert C.ws_bytes(2, 273, 2) == 13312 and C.ws_bytes(1, 1, 1) == 256 and C.ws_bytes(16, 499, 12) == 3 * 16 * 12 * 499 * 4
    assert [f[:2] for f in C.FRAMES] == [(513, 1), (513, 256), (513, 17)] and [f[2] for f in C.FRAMES] == [257, 273, 129]
    assert all(c[1] == C.FRAMES_T == 513 and c[4] == 3 for c in C.FRAME_CASES)
    assert {c[3] for c in C.FRAME_CASES} == {24, 40, 64, 120} and {c[0] for c in C.FRAME_CASES} == set(C.ENTRIES)


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.KIND_SHAPES, ids=str)
def test_ordered_maxima_sit_in_their_blocks(entry, shape):
    """Three key blocks of the query kernel's size; the row maximum of query i lies in block i % 3, the best score of each other
    block at least 40 below it; for target 2 the running maximum rises twice; q and k are multiples of 1/8."""
    T, heads, dm, B = shape
    ref = C.reference("ordered", entry, *shape)
    assert C.instances_of(entry, T, dm)[0][2] == 3
    for t in (ref["q"], ref["k"]):
        assert torch.equal(t * 8.0, torch.round(t * 8.0))
    s = C.scores(ref)
    blk, tgt = AL.ordered_block(T, C.KB), AK.ordered_target(T)
    assert sorted(set(blk.tolist())) == [0, 1, 2] and all((tgt == c).sum().item() >= T // 3 for c in range(3))
    best = torch.stack([s[..., blk == c].max(-1).values for c in range(3)], -1)
    assert torch.equal(best.argmax(-1), tgt.expand(B, heads, T))
    own = best.gather(-1, tgt.expand(B, heads, T).unsqueeze(-1))
    others = best.masked_fill(torch.nn.functional.one_hot(tgt, 3).bool().expand_as(best), float("-inf"))
    margin = (own - others.max(-1, keepdim=True).values).min().item()
    print(f"ordered {entry} {shape}: smallest margin {margin:.2f}, max|score| {s.abs().max().item():.2f}")
    assert margin >= AK.ORDERED_GAP
    rise = best[..., tgt == 2, :]
    assert (rise[..., 0] < rise[..., 1]).all() and (rise[..., 1] < rise[..., 2]).all()
    assert (s.max(-1).values - s.min(-1).values).min().item() > 40 and s.abs().max().item() < 30.0


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.KIND_SHAPES, ids=str)
def test_uniform_probabilities_are_one_over_t(entry, shape):
    ref = C.reference("uniform", entry, *shape)
    assert not ref["q"].any()
    assert (ref["P"] - 1.0 / shape[0]).abs().max().item() <= 2.0 ** -53
    H = shape[1] * shape[2]
    assert not ref["plain"][:, H:2 * H].any()                                            # dk = dS^T q = 0


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.KIND_SHAPES, ids=str)
def test_peaked_rows_are_peaked(entry, shape):
    """Row maxima above 0.999 on the diagonal, scores that span more than 40 and are no larger than that asks for, exact q . k."""
    ref = C.reference("peaked", entry, *shape)
    s = C.scores(ref)
    top = ref["P"].max(-1)
    assert top.values.min().item() > 0.999
    assert torch.equal(top.indices, torch.arange(shape[0]).expand_as(top.indices))
    assert (s.max(-1).values - s.min(-1).values).min().item() > AK.PEAK_SPAN > 39.9
    assert s.abs().max().item() < AK.PEAK_SCORE * 1.05
    assert torch.equal(ref["k"] * 8.0, torch.round(ref["k"] * 8.0)) and torch.equal(ref["q"], 4.0 * ref["k"])


@pytest.mark.parametrize("s", [x for x in C.all_input_sets() if x[0] != "random" or (x[2] == 273 and x[4] in C.INSTANCE_DIMS)], ids=AK.set_id)
def test_bars_are_within_reach_of_fp32(s):
    """A plain numpy fp32 restatement stays within half the entry's bar on these inputs, each third against its own maximum, and
    the split rounding of the fp64 result within a tenth of the split bar."""
    kind, entry, T, heads, dm, B = s
    qkv, dctx = C.inputs(kind, entry, T, heads, dm, B)
    ref = C.reference(kind, entry, T, heads, dm, B)
    H = heads * dm
    np32 = C.third_errors(C.attention_bwd_np32(qkv, dctx, B, T, heads, dm), ref["plain"], H)
    bar = C.TOL_F16 if entry == "f16" else C.TOL_SPLIT
    print(f"{AK.set_id(s)}: numpy fp32 rel err dq {np32[0]:.2e} dk {np32[1]:.2e} dv {np32[2]:.2e} (bar {bar:.2e})")
    assert max(np32) <= 0.5 * bar, np32
    if entry == "split":
        hi, lo, over = split_ref(ref["plain"])
        assert not over.any()
        assert max(C.third_errors(hi.double() + lo.double() / 2048.0, ref["plain"], H)) <= 0.1 * C.TOL_SPLIT


def test_linear_inputs_hold_their_precondition():
    qkv, dctx = C.linear_inputs()
    assert torch.equal(qkv, qkv.half().double()) and torch.equal(dctx, dctx.half().double())      # fp16-exact: lo planes are zero
    lo, hi = C.linear_precondition(qkv, dctx)
    print(f"linear inputs: nonzero |outputs| over both scaled launches in [{lo:.3e}, {hi:.3e}]")
    assert C.LINEAR_RANGE[0] <= lo and hi <= C.LINEAR_RANGE[1]
    T, heads, dm, B = C.LINEAR_SHAPE
    assert T == 273 and all(l >= 3 for _, _, l, _ in C.instances_of("split", T, dm))
