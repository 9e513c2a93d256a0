"""CPU-only: the kernels of csrc/influence.hip compile without scratch (register spills), read from hipcc's kernel-resource
remarks as tests/test_build_resources.py does.  The moment kernel holds four MFMA accumulators, the squared-distance kernel
sixteen fp32 chains and eight staged float4; a spill there would turn a memory-bound launch into a scratch-bound one that no
parity test sees."""
from test_build_resources import resources

KERNELS = ("moment_partial_kernel", "sqdist_partial_kernel", "gram_fold_kernel", "sumsq_kernel", "residual_kernel", "cosine_kernel",
           "scale_kernel", "self_scale_kernel", "topk_pass_kernel")


def test_influence_kernels_do_not_spill():
    res = resources("influence.hip")
    assert all(any(name in k for name in KERNELS) for k in res), sorted(res)   # every kernel of the file is listed above
    for name in KERNELS:
        hit = {k: v for k, v in res.items() if name in k}
        assert hit, (name, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    for name in ("moment_partial_kernel", "sqdist_partial_kernel"):
        tiled = {k: v for k, v in res.items() if name in k}
        assert len(tiled) == 2, sorted(res)                                  # the 16-byte and the 4-byte staging instance
        for k, v in tiled.items():
            assert v["occupancy"] >= 2, (k, v)                               # two workgroups per CU cover each other's staging
