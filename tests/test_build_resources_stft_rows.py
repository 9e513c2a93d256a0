"""CPU-only: the row-mapped STFT instantiations (csrc/stft.hip: ``istft_kernel<4, FB>`` and ``stft_fwd_kernel<FB, 2>``, the
launches of advh_istft_masked_rows / advh_istft_masked_rows_bwd) against their siblings ``istft_kernel<3, FB>`` and
``stft_fwd_kernel<FB, 1>`` in the same compile, by the method of test_build_resources.py (hipcc's kernel-resource remarks).

At FB = 8, the value every caller runs unless ``stft_frames_per_workgroup`` is set to 16, both are free of scratch.  At FB = 16
the shared template code itself spills in every instantiation, old and new (232 bytes per lane in each ``istft_kernel<*, 16>``,
440 in ``stft_fwd_kernel<16, 1>``, 456 in ``<16, 0>``: the 17 tile registers per thread of the inverse under its 128-VGPR bound,
the two frames per wavefront of the forward under its 80); the new instantiations are that shared code, so there they are held
to their sibling's figure: no byte of scratch more.  Occupancy is at least the sibling's at both FB."""
import pytest

from test_build_resources import resources


@pytest.fixture(scope="module")
def stft():
    res = resources("stft.hip")

    def find(kernel, a, b):
        hit = [v for k, v in res.items() if f"{kernel}ILi{a}ELi{b}E" in k]
        assert len(hit) == 1, (kernel, a, b, sorted(res))
        return hit[0]
    return find


@pytest.mark.parametrize("FB", [8, 16])
def test_row_mapped_instantiations_match_their_siblings(stft, FB):
    for new, old in ((stft("istft_kernel", 4, FB), stft("istft_kernel", 3, FB)),
                     (stft("stft_fwd_kernel", FB, 2), stft("stft_fwd_kernel", FB, 1))):
        print(FB, new, old)
        assert new["scratch"] <= old["scratch"], (FB, new, old)
        assert new["occupancy"] >= old["occupancy"], (FB, new, old)


def test_row_mapped_instantiations_have_no_scratch_at_the_default_tile(stft):
    assert stft("istft_kernel", 4, 8)["scratch"] == 0
    assert stft("stft_fwd_kernel", 8, 2)["scratch"] == 0
