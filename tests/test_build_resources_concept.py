"""CPU-only: the kernels of csrc/concept.hip compile without scratch (register spills), read from hipcc's kernel-resource
remarks as tests/test_build_resources.py does.  The Gram kernel holds four MFMA accumulators and its staging registers; a spill
there would turn a memory-bound launch into a scratch-bound one that no parity test sees."""
from test_build_resources import resources


def test_concept_kernels_do_not_spill():
    res = resources("concept.hip")
    gram = {k: v for k, v in res.items() if "gram_partial_kernel" in k}
    assert len(gram) == 2, sorted(res)                                       # the 16-byte and the 4-byte staging instance
    for name in ("gram_partial_kernel", "gram_fold_kernel", "combine_kernel", "time_pool_kernel"):
        hit = {k: v for k, v in res.items() if name in k}
        assert hit, (name, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    for k, v in gram.items():
        assert v["occupancy"] >= 2, (k, v)                                   # two workgroups per CU cover each other's staging
