"""CPU-only: csrc/stft_ragged.hip and csrc/unet_ragged.hip compile for gfx950 without scratch and without atomics, and the two
STFT-class kernels keep at least the occupancy (waves per SIMD) of the kernels of csrc/stft.hip whose arithmetic they carry,
``stft_fwd_kernel<FB, 0>`` and ``istft_kernel<3, FB>``, compiled here from stft.hip for the comparison.  The VGPR counts are
printed; DESIGN 4.37 records them."""
import os

from test_build_resources import CSRC
from test_build_resources_backward import instances, resources


def by_instance(res, kernel, args):
    tag = "I" + "".join(f"Li{a}E" for a in args) + "E"
    hit = [v for k, v in res.items() if kernel in k and tag in k]
    assert len(hit) == 1, (kernel, args, sorted(res))
    return hit[0]


def test_the_ragged_stft_kernels_keep_their_siblings_occupancy_without_scratch():
    new, old = resources("stft_ragged.hip"), resources("stft.hip")
    assert instances("stft_ragged.hip", "stft_fwd_ragged_kernel") == {("stft_fwd_ragged_kernel", 8), ("stft_fwd_ragged_kernel", 16)}
    assert instances("stft_ragged.hip", "istft_c64_ragged_kernel") == {("istft_c64_ragged_kernel", 8), ("istft_c64_ragged_kernel", 16)}
    assert len([k for k in new if "_kernel" in k]) == 4, sorted(new)
    for fb in (8, 16):
        for mine, sibling in ((by_instance(new, "stft_fwd_ragged_kernel", (fb,)), by_instance(old, "stft_fwd_kernel", (fb, 0))),
                              (by_instance(new, "istft_c64_ragged_kernel", (fb,)), by_instance(old, "istft_kernel", (3, fb)))):
            print(f"FB = {fb}: ragged {mine}, sibling {sibling}")
            assert mine["scratch"] == 0, (fb, mine)                          # some siblings keep a few spilled loop invariants
            assert mine["occupancy"] >= sibling["occupancy"], (fb, mine, sibling)


def test_the_tail_kernels_use_no_scratch():
    res = {k: v for k, v in resources("unet_ragged.hip").items() if "_kernel" in k}
    assert len(res) == 2 and any("fmap_clip_tail_kernel" in k for k in res) and any("zero_tail_cols_f32_kernel" in k for k in res), sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)


def test_the_new_files_have_no_atomics():
    for src in ("stft_ragged.hip", "unet_ragged.hip"):
        text = open(os.path.join(CSRC, src)).read()
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        code = code.replace("__ATOMIC_ACQ_REL", "")                          # the memory order of the wavefront fence: no atomic operation
        assert "atomic" not in code.lower(), src
