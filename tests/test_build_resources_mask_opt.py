"""CPU-only: the kernels of csrc/mask_opt.hip compile without scratch (register spills), read from hipcc's kernel-resource
remarks as tests/test_build_resources.py does.  The step kernel's footprint search and the rows kernel's four-lane pack are the
places where a runtime-indexed array or an unrolled loop could spill; all three sit inside the optimisation loop."""
from test_build_resources import resources

KERNELS = ("mask_opt_rows_kernel", "mask_opt_terms_kernel", "mask_opt_step_kernel")


def test_mask_opt_kernels_do_not_spill():
    res = resources("mask_opt.hip")
    assert all(any(name in k for name in KERNELS) for k in res), sorted(res)   # every kernel of the file is listed above
    for name in KERNELS:
        hit = {k: v for k, v in res.items() if name in k}
        assert hit, (name, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    assert len([k for k in res if "mask_opt_rows_kernel" in k]) == 2           # the float4 and the scalar form
