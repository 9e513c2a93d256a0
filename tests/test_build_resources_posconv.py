"""CPU-only: register budget of the positional convolution's line tile (csrc/posconv_tile.hip), read off hipcc's
kernel-resource remarks.  The host launches two workgroups of four wavefronts per CU whenever the LDS need allows
(advh_posconv_tile_f16: ``per_cu``), so both instances must keep an occupancy of two waves per SIMD; a change that pushes the
48-channel instance into spilling, or grows the spill of the 64-channel one, shows in no parity test."""
from test_build_resources_backward import instances, resources


def test_posconv_tile_register_budget():
    res = {k: v for k, v in resources("posconv_tile.hip").items() if "posconv_tile_kernel" in k}
    assert instances("posconv_tile.hip", "posconv_tile_kernel") == {("posconv_tile_kernel", 6), ("posconv_tile_kernel", 8)}
    assert len(res) == 2, sorted(res)
    for name, v in res.items():
        assert v["occupancy"] >= 2, (name, v)
        if "ILi6E" in name:
            assert v["scratch"] == 0, (name, v)                    # 48 channels per group: 209 VGPRs, nothing spilled
        else:
            # 64 channels per group: 256 VGPRs and 12 bytes per lane of scratch at the commit that added this test; removing
            # them is performance work of its own, growing them is a regression
            assert v["scratch"] <= 12, (name, v)
