"""CPU-only: every compiled instance of the attention-backward and LayerNorm-backward kernels is selected by a case of
tests/test_gpu_backward_kernels.py, and the cases select nothing that is not compiled.  The template arguments are read off
the mangled kernel names in hipcc's resource remarks; a new or dropped instantiation fails here until the case lists follow."""
import functools
import re

import backward_kernel_cases as K
from test_build_resources import resources as _resources

resources = functools.lru_cache(maxsize=None)(_resources)            # backward.hip is compiled once for both tests


def instances(src, kernel):
    """{(kernel, arg, ...)} of ``kernel``'s instantiations in ``src``: Itanium-mangled integer (Li<n>E) and bool (Lb<0|1>E) arguments."""
    out = set()
    for name in resources(src):
        m = re.search(rf"\d+{kernel}I((?:L[ib]\d+E)+)E", name)
        if m:
            out.add((kernel,) + tuple(bool(int(v)) if t == "b" else int(v) for t, v in re.findall(r"L([ib])(\d+)E", m.group(1))))
    return out


def test_every_attention_bwd_instance_has_a_case():
    sets = [instances("backward.hip", "attention_bwd_kernel"), instances("attention_bwd_x3.hip", "attention_bwd_x3_kernel"),
            instances("attention_bwd_f32.hip", "attention_bwd_f32_kernel")]
    # the last template argument is RAGGED: the batch set here, the ragged one in tests/test_build_resources_attention_bwd_ragged.py
    assert [sum(not i[-1] for i in s) for s in sets] == [15, 8, 12], [sorted(s) for s in sets]
    compiled = {i for s in sets for i in s if not i[-1]}
    selected = K.att_selected()
    refused = {K.instance_of("f16", T, dm) for T, dm in K.REFUSED_CASES}
    assert refused == {("attention_bwd_kernel", 16, 128, False, False)}    # compiled, but its LDS need is above 160 KiB: never launched
    assert all(K.refused_f16(T, dm) for T, dm in K.REFUSED_CASES)
    assert not refused & set(selected)
    assert set(selected) | refused == compiled, (sorted(compiled - set(selected) - refused), sorted(set(selected) - compiled))
    for inst, cases in selected.items():
        kernel, NT, D, last, _ = inst
        lo, hi = {4: (1, 64), 8: (65, 128), 13: (129, 208), 16: (209, 256)}[NT]
        if kernel == "attention_bwd_kernel" and D == 128 and NT == 13:
            lo = 65                                                         # head dim 128 has no 8-tile instance
        Ts = {c[1] for c in cases}
        assert {lo, hi} <= Ts, (inst, sorted(Ts))                           # both edges of the tile-count class
        if not (kernel == "attention_bwd_kernel" and last):                 # the transposing path takes head dim 64 only
            assert any(c[3] < D and c[2] >= 2 for c in cases), inst         # a padded head dim next to a neighbouring head


def test_every_layernorm_bwd_instance_has_a_case():
    compiled = instances("backward.hip", "layernorm_bwd_kernel")
    assert len(compiled) == 12, sorted(compiled)
    selected = {}
    for c in K.LN_CASES:
        selected.setdefault(("layernorm_bwd_kernel",) + K.ln_instance_of(c["x"], c["dy"], c["C"]), []).append(c)
    assert set(selected) == compiled, (sorted(compiled - set(selected)), sorted(set(selected) - compiled))
    for inst, cases in selected.items():
        assert {c["gelu"] for c in cases} == {0, 1}, inst
        assert any(c["dact"] for c in cases) and any(c["add"] for c in cases), inst
        assert {c["out"] for c in cases} == {"f", "h", "fh"}, inst
    assert {c["C"] for c in K.LN_CASES} == set(K.LN_C) and {c["M"] for c in K.LN_CASES} == set(K.LN_M)
    assert {c["dact"] for c in K.LN_CASES} == {None, "f16", "split"}
    assert {c["x"] for c in K.LN_CASES} == {c["dy"] for c in K.LN_CASES} == {"f32", "f16", "split"}
