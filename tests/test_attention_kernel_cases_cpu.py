"""CPU-only: the preconditions of the inputs of tests/test_gpu_attention_kernels.py, asserted from the fp64 reference and never
from a kernel, and the proof that the bars of that module are within reach of fp32 arithmetic on exactly these inputs: if a
check here fails, the inputs change, not the bars."""
import pytest
import torch

import attention_kernel_cases as K
from split_contract_ref import split_ref


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.PEAKED_SHAPES, ids=str)
def test_peaked_rows_are_peaked(entry, shape):
    """Every row maximum of P exceeds 0.999, sits on the diagonal, and the row's scores span more than 40."""
    ref = K.reference("peaked", entry, *shape)
    s = K.scores(ref)
    top = ref["p"].max(-1)
    assert top.values.min().item() > 0.999
    assert torch.equal(top.indices, torch.arange(shape[0]).expand_as(top.indices))
    assert (s.max(-1).values - s.min(-1).values).min().item() > K.PEAK_SPAN
    assert s.abs().max().item() < K.PEAK_SCORE * 1.01                 # no score larger than the span asks for


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_ordered_maxima_sit_in_their_blocks(entry):
    """The row maximum of query i lies in key block i % 3, the best score of each other block at least 40 below it; for
    target 2 the running maximum rises twice (block 0 < block 1 < block 2)."""
    T, heads, dm, B = K.ORDERED_SHAPE
    s = K.scores(K.reference("ordered", entry, T, heads, dm, B))                  # [B, heads, T, T]
    blk, tgt = K.ordered_block(T), K.ordered_target(T)
    assert sorted(set(blk.tolist())) == [0, 1, 2] and all((tgt == c).sum().item() >= T // 3 for c in range(3))
    best = torch.stack([s[..., blk == c].max(-1).values for c in range(3)], -1)   # [B, heads, T, 3]: best score per key block
    assert torch.equal(best.argmax(-1), tgt.expand(B, heads, T))
    own = best.gather(-1, tgt.expand(B, heads, T).unsqueeze(-1))
    others = best.masked_fill(torch.nn.functional.one_hot(tgt, 3).bool().expand_as(best), float("-inf"))
    margin = (own - others.max(-1, keepdim=True).values).min().item()
    print(f"ordered [{entry}]: smallest margin of the target block {margin:.2f}, max|score| {s.abs().max().item():.2f}")
    assert margin >= K.ORDERED_GAP
    rise = best[..., tgt == 2, :]
    assert (rise[..., 0] < rise[..., 1]).all() and (rise[..., 1] < rise[..., 2]).all()
    assert s.abs().max().item() < 30.0                                            # no larger than the margin asks for


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.UNIFORM_SHAPES, ids=str)
def test_uniform_probabilities_are_one_over_t(entry, shape):
    ref = K.reference("uniform", entry, *shape)
    T = shape[0]
    assert not ref["q"].any()
    assert (ref["p"] - 1.0 / T).abs().max().item() <= 2.0 ** -53
    assert (ref["ctx"] - ref["v"].mean(-2, keepdim=True)).abs().max().item() <= 1e-14


def test_adversarial_shapes_reach_every_template():
    for kind, shapes in K.KIND_SHAPES.items():
        if kind == "ordered":
            assert K.instance_of("split", *K.ORDERED_SHAPE[::2])[3:] == (3, 2)     # three key blocks, two query rounds
            continue
        for entry in K.ENTRIES:
            assert {K.instance_of(entry, s[0], s[2])[0] for s in shapes} == K.TEMPLATES[entry], (kind, entry)
    assert {s[0] for s in K.UNIFORM_SHAPES} == {17, 113, 209, 225}


def test_head_scales_are_exact_powers_of_two():
    """Head h of V carries HEAD_SCALE[h]: in both formats the scaled values are the unscaled ones times that power of two."""
    T, heads, dm, B = 65, 3, 40, 3
    for fmt in K.ENTRIES:
        v = K.reference("random", fmt, T, heads, dm, B)["v"]
        tops = v.abs().amax((0, 2, 3))
        assert tops[1] < tops[0] / 2 and tops[2] > tops[0] * 2


@pytest.mark.parametrize("s", K.all_input_sets(), ids=K.set_id)
def test_bars_are_within_reach_of_fp32(s):
    """Per (clip, head) block, against the fp64 reference on the values the kernel reads:
      * the split rounding of the fp64 result by itself (split_contract_ref.split_ref) stays within a tenth of the split bar;
      * a plain numpy fp32 restatement of softmax(Q K^T / sqrt(d)) V stays within half the split bar."""
    kind, entry, T, heads, dm, B = s
    ref = K.reference(kind, entry, T, heads, dm, B)
    np32 = K.split_ratio(K.attention_np32(ref["q"], ref["k"], ref["v"]), ref["ctx"])
    print(f"{K.set_id(s)}: numpy fp32 |err| / split bar {np32:.3f}")
    assert np32 <= 0.5, np32
    if entry == "split":
        hi, lo, over = split_ref(ref["ctx"])
        assert not over.any()
        rounding = K.split_ratio(hi.double() + lo.double() / 2048.0, ref["ctx"])
        assert rounding <= 0.1, rounding
