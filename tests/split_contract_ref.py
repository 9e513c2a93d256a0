"""fp64 restatement of the split format's range contract (csrc/device_math.h, include/addvisor_hip.h advh_split_overflow) for
tests/test_split_contract_cpu.py and tests/test_gpu_split_contract.py.

An fp32 value x travels as two fp16 planes with x = hi + lo * 2^-11:

  |x| <= 65504            hi = fp16(x), or +0 when |x| < 2^-14; lo = fp16((x - hi) * 2^11)          flag: no
  |x| > 65504, +-inf      hi = +-65504; lo = fp16 of (x - hi) * 2^11 clamped to +-65504 (saturates)  flag: YES
  NaN                     hi = lo = NaN                                                             flag: no

For an fp32 x the difference x - hi is exact in fp32 and in fp64, so the single rounding to fp16 here is the device's."""
import numpy as np
import torch

SPLIT_MAX = 65504.0
TINY = 2.0 ** -14

# the edge values every producer test places (tests/test_gpu_split_contract.py)
EDGE_IN_RANGE = [0.0, -0.0, TINY, -TINY, TINY * (1 - 2.0 ** -12), -TINY * (1 - 2.0 ** -12), 3e-8, -3e-8, 65504.0, -65504.0]
EDGE_OUT_OF_RANGE = [65504.5, -65504.5, 65519.9, 65520.0, -65520.0, 65535.98, -65535.98, 65536.0, 1e5, -1e5,
                     float("inf"), float("-inf")]
EDGE_NAN = [float("nan")]
EDGE_VALUES = EDGE_IN_RANGE + EDGE_OUT_OF_RANGE + EDGE_NAN


def split_ref(x):
    """``(hi, lo, flagged)`` the contract requires for the fp32 values ``x`` (array-like): fp16 tensors of x's shape and a bool
    tensor, True where the value is out of range (the producing launch must raise the sticky flag iff any is True)."""
    x = torch.as_tensor(x).to(torch.float32).to(torch.float64).numpy()
    nan = np.isnan(x)
    over = ~nan & (np.abs(x) > SPLIT_MAX)
    hi = np.where(over, np.copysign(SPLIT_MAX, x), x)
    hi = np.where(np.abs(x) < TINY, 0.0, hi).astype(np.float16)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (x - hi.astype(np.float64)) * 2048.0
    r = np.where(over, np.clip(r, -SPLIT_MAX, SPLIT_MAX), r)
    with np.errstate(over="ignore"):
        lo = r.astype(np.float16)
    hi = np.where(nan, np.float16(np.nan), hi)
    lo = np.where(nan, np.float16(np.nan), lo)
    return torch.from_numpy(hi.copy()), torch.from_numpy(lo.copy()), torch.from_numpy(over)


def split_ref_planes(x) -> torch.Tensor:
    """``split_ref`` as one fp16 plane pair ``[2, *x.shape]``."""
    hi, lo, _ = split_ref(x)
    return torch.stack([hi, lo])


def same_planes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Plane-for-plane equality with NaN == NaN (any payload) and +0 == -0 kept apart only by ``same_bits``."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    return bool(torch.equal(na, nb) and torch.equal(a[~na], b[~nb]))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-identical fp16 tensors (signed zeros and NaN payloads included)."""
    return bool(torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16)))
