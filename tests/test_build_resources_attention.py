"""CPU-only: every compiled instance of the five forward attention kernel templates (csrc/attention.hip) is selected by a
parity case of tests/test_gpu_attention_kernels.py, at both edges of its tile-count class, and the cases select nothing that
is not compiled.  The template arguments are read off the mangled kernel names in hipcc's resource remarks; a new or dropped
instantiation fails here until tests/attention_kernel_cases.py follows."""
import attention_kernel_cases as K
from test_build_resources_backward import instances

F16 = ("attention_tr_kernel", "attention_kernel")
SPLIT = ("attention_x3_tr_kernel", "attention_x3_kernel", "attention_x3_stream_kernel")


def compiled(kernels):
    return set().union(*(instances("attention.hip", k) for k in kernels))


def check_reach(selected, stream):
    """What the case table owes every selected instance."""
    for inst, cases in selected.items():
        kernel, NT = inst[0], inst[1]
        D = inst[2] if len(inst) > 2 else 64
        if kernel != "attention_x3_stream_kernel":
            lo, hi = K.CLASSES[NT]
            if inst == ("attention_kernel", 13, 128):
                lo = 65                                                      # head dim 128 has no 8-tile instance
            Ts = {c[1] for c in cases}
            assert {lo, hi} <= Ts, (inst, sorted(Ts))                        # both edges of the tile-count class
            assert all(lo <= t <= hi for t in Ts), (inst, sorted(Ts))
        if kernel not in ("attention_tr_kernel", "attention_x3_tr_kernel"):  # the transposing kernels take head dim 64 only
            padded = {c[3] for c in cases if c[3] < D and c[2] >= 2}         # a padded head dim next to a neighbouring head
            assert padded, inst
            if D == 128:
                assert {72, 120} <= padded, (inst, sorted(padded))
    assert {blocks for blocks, _ in stream} == {1, 2, 3} and {rounds for _, rounds in stream} == {1, 2}, sorted(stream)


def test_every_attention_instance_has_a_case():
    f16, split = compiled(F16), compiled(SPLIT)
    assert len(instances("attention.hip", "attention_tr_kernel")) == 4 and len(instances("attention.hip", "attention_kernel")) == 11, sorted(f16)
    assert [len(instances("attention.hip", k)) for k in SPLIT] == [4, 8, 1], sorted(split)
    selected = K.att_selected()
    assert set(selected) == f16 | split, (sorted((f16 | split) - set(selected)), sorted(set(selected) - (f16 | split)))
    assert {i for i, cs in selected.items() if any(c[0] == "f16" for c in cs)} == f16         # each entry reaches its own kernels
    assert {i for i, cs in selected.items() if any(c[0] == "split" for c in cs)} == split
    check_reach(selected, K.stream_reach())


def test_dispatch_mirror_at_the_class_edges():
    """The mirror itself, spelled out where the classes meet (csrc/attention.hip, advh_attention_f16 / advh_attention_split)."""
    assert K.instance_of("f16", 64, 64) == ("attention_tr_kernel", 4) and K.instance_of("f16", 65, 64) == ("attention_tr_kernel", 8)
    assert K.instance_of("split", 208, 64) == ("attention_x3_tr_kernel", 13) and K.instance_of("split", 209, 64) == ("attention_x3_tr_kernel", 16)
    assert K.instance_of("f16", 128, 56) == ("attention_kernel", 8, 64) and K.instance_of("f16", 129, 8) == ("attention_kernel", 13, 32)
    assert K.instance_of("f16", 64, 72) == ("attention_kernel", 4, 128) and K.instance_of("f16", 65, 72) == ("attention_kernel", 13, 128)
    assert K.instance_of("f16", 128, 128) == ("attention_kernel", 13, 128) and K.instance_of("f16", 256, 120) == ("attention_kernel", 16, 128)
    assert K.instance_of("split", 129, 32) == ("attention_x3_kernel", 13, 32) and K.instance_of("split", 208, 24) == ("attention_x3_kernel", 13, 32)
    assert K.instance_of("split", 112, 72) == ("attention_x3_stream_kernel", 7, 128, 1, 1)
    assert K.instance_of("split", 113, 128) == ("attention_x3_stream_kernel", 7, 128, 2, 1)
    assert K.instance_of("split", 129, 120) == ("attention_x3_stream_kernel", 7, 128, 2, 2)
    assert K.instance_of("split", 225, 120) == ("attention_x3_stream_kernel", 7, 128, 3, 2)
