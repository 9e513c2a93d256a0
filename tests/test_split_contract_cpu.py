"""The fp64 model of the split format's range contract (tests/split_contract_ref.py) against the host packer
``gemm.split_planes`` on in-range values, and the model's own out-of-range / NaN rows (include/addvisor_hip.h advh_split_overflow)."""
import math

import numpy as np
import pytest
import torch

from addvisor_hip import gemm as G
from split_contract_ref import EDGE_IN_RANGE, EDGE_NAN, EDGE_OUT_OF_RANGE, EDGE_VALUES, SPLIT_MAX, TINY, same_bits, split_ref


def test_split_ref_matches_host_packer_in_range():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 40, generator=g) * torch.logspace(-10, 4.8, 40)[None, :]
    x = x.clamp(-SPLIT_MAX, SPLIT_MAX)
    edge = torch.tensor(EDGE_IN_RANGE + [TINY * (1 + 2.0 ** -10), -TINY * (1 + 2.0 ** -10), 1e-45, -1e-45, 65503.99])
    for t in (x.reshape(-1), edge):
        hi, lo, flagged = split_ref(t)
        host = G.split_planes(t)
        assert not flagged.any()
        assert same_bits(hi, host[0]) and same_bits(lo, host[1])          # bit for bit, signed zeros included
        assert (G.join_planes(torch.stack([hi, lo])).double() - t.double()).abs().le(
            torch.maximum(t.double().abs() * 2.0 ** -21, torch.full_like(t.double(), 2.0 ** -25))).all()


def test_split_ref_rows_of_the_contract():
    hi, lo, flagged = split_ref(torch.tensor([0.0, -0.0, TINY, TINY * (1 - 2.0 ** -12), 3e-8]))
    assert hi.view(torch.int16).tolist()[:2] == [0, 0]                    # +0 hi below 2^-14, the sign lives in lo
    assert lo.view(torch.int16).tolist()[:2] == [0, -32768]
    assert float(hi[2]) == TINY and float(lo[2]) == 0.0
    assert float(hi[3]) == 0.0 and float(lo[3]) == float(np.float16(np.float32(TINY * (1 - 2.0 ** -12)) * 2048.0))
    assert float(hi[4]) == 0.0 and float(lo[4]) == float(np.float16(np.float32(3e-8) * 2048.0))
    assert not flagged.any()
    x = torch.tensor(EDGE_OUT_OF_RANGE)
    hi, lo, flagged = split_ref(x)
    assert flagged.all() and torch.equal(hi.float().abs(), torch.full_like(x, SPLIT_MAX))
    assert torch.equal(torch.sign(hi.float()), torch.sign(x)) and torch.isfinite(lo.float()).all()
    joined = G.join_planes(torch.stack([hi, lo]))
    assert (joined.abs() <= 65535.984375).all()
    exact = x.abs() <= 65535.98                                             # saturation keeps x up to 65535.98 (to lo's rounding)
    assert ((joined - x).abs()[exact] <= 16.0 / 2048).all()
    assert (joined[~exact].abs() == 65535.984375).all()
    assert float(joined[EDGE_OUT_OF_RANGE.index(65504.5)]) == 65504.5
    hi, lo, flagged = split_ref(torch.tensor(EDGE_NAN))
    assert math.isnan(float(hi[0])) and math.isnan(float(lo[0])) and not flagged.any()
    assert len(EDGE_VALUES) == len(EDGE_IN_RANGE) + len(EDGE_OUT_OF_RANGE) + len(EDGE_NAN)


@pytest.mark.parametrize("bad", [65504.5, float("inf"), float("nan")])
def test_host_packer_refuses_what_the_device_saturates(bad):
    with pytest.raises(ValueError):
        G.split_planes(torch.tensor([1.0, bad]))
