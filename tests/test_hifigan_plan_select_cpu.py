"""CPU-only: which kernel every layer of the HiFi-GAN generator gets (``gemm.select_conv1d`` / ``gemm.select_resblock_step`` under
``HipHifigan``'s stage policy), for all sixteen combinations of precision x line_tile x fuse x padding_mode.  ``HipHifigan._workspace``
plans on the CPU once ``_lib.init`` is stubbed: plans are host objects until ``run``."""
from collections import Counter

import pytest
import torch

from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.hifigan import HipHifigan

GEMM, HALO, MIX = ("gemm", "GemmPlan", "gemm"), ("halo", None, None), ("mix", None, None)
TAPS = {"f16": ("gemm", "TapsPlan", "taps"), "f32": ("gemm", "TapsPlan", "taps_x3")}
PAIR = {"f16": ("gemm", "ResblockPairPlan", "resblock_pair"), "f32": ("gemm", "ResblockPairX3Plan", "resblock_pair_x3")}
# ws["flops"] at (1, 8): the GEMMs enumerate their halo rows, the tile kernels count valid positions only
FLOPS = {"v1": {"gemm": 6358646784, "f16": 6276071424, "f32": 6280790016},
         "tiny": {"gemm": 397071360, "f16": 314496000, "f32": 319214592}}
CONFIGS = {"tiny": syn.hifigan_tiny_config, "v1": syn.HifiganConfig}


def expected(cfg, precision, line_tile, fuse, padding_mode):
    """``(step kind, plan class, plan kind)`` of every step, and which ``FLOPS`` column the network is.  "reflect" leaves the implicit
    GEMM only; in "f32" ``line_tile`` is ignored and ``fuse`` gates the fused 32-channel step and the 64-channel split line tile
    (first convolutions from k = 3, second ones from k = 7); in "f16" ``fuse`` needs ``line_tile``, and two 64-channel k = 11 weight
    tensors do not fit in LDS."""
    reflect = padding_mode == "reflect"
    tile = not reflect and (fuse if precision == "f32" else line_tile)
    nd = len(cfg.resblock_dilations)
    steps = [HALO] * reflect + [GEMM]                                       # conv_pre
    co = cfg.upsample_initial_channel
    for _ in cfg.upsample_rates:
        co //= 2
        steps += [GEMM] + [HALO, HALO] * reflect                            # the up-sampler, then x and lrelu(x)
        for k in cfg.resblock_kernel_sizes:
            for d in range(nd):
                if precision == "f16":
                    pair = tile and fuse and (co == 32 or (co == 64 and k <= 7))
                    conv1 = conv2 = TAPS["f16"] if tile and co in (32, 64) else GEMM
                else:
                    pair = tile and co == 32
                    conv1 = TAPS["f32"] if tile and co == 64 else GEMM
                    conv2 = TAPS["f32"] if tile and co == 64 and k >= 7 else GEMM
                steps += [PAIR[precision]] if pair else [conv1] + [HALO] * reflect + [conv2] + [HALO] * (reflect and d < nd - 1)
        steps += [MIX] + [HALO] * reflect
    return steps, (precision if tile else "gemm")


def check(name, precision, line_tile, fuse, padding_mode):
    cfg = CONFIGS[name]()
    net = HipHifigan(cfg, syn.hifigan_weights(cfg), torch.device("cpu"), line_tile=line_tile, fuse=fuse, padding_mode=padding_mode,
                     precision=precision)
    ws = net._workspace(1, 8)
    want, column = expected(cfg, precision, line_tile, fuse, padding_mode)
    got = [(s[0],) + ((type(s[1]).__name__, s[1].kind) if s[0] == "gemm" else (None, None)) for s in ws["steps"]]
    assert got == want
    assert [s.kind for s in ws["steps"]] == [w[0] for w in want]            # the records' named fields
    assert ws["flops"] == FLOPS[name][column]
    return Counter((cls or kind) + ("/x3" if cls == "TapsPlan" and pk == "taps_x3" else "") for kind, cls, pk in got)


# the table of the six distinct networks: step count and contents, the same for the tiny and the V1 configuration
ROWS = {
    "reflect": dict(GemmPlan=77, halo=73, mix=4),
    "gemm": dict(GemmPlan=77, mix=4),
    "f16 taps": dict(GemmPlan=41, TapsPlan=36, mix=4),
    "f16 fused": dict(GemmPlan=41, ResblockPairPlan=15, TapsPlan=6, mix=4),
    "f32 fused": {"GemmPlan": 44, "ResblockPairX3Plan": 9, "TapsPlan/x3": 15, "mix": 4},
}
STEPS = {"reflect": 154, "gemm": 81, "f16 taps": 81, "f16 fused": 66, "f32 fused": 72}


def row(precision, line_tile, fuse, padding_mode):
    if padding_mode == "reflect":
        return "reflect"
    if precision == "f32":
        return "f32 fused" if fuse else "gemm"
    return ("f16 fused" if fuse else "f16 taps") if line_tile else "gemm"


@pytest.mark.parametrize("padding_mode", ["zeros", "reflect"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("line_tile", [False, True])
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_hifigan_plan_table(monkeypatch, precision, line_tile, fuse, padding_mode):
    monkeypatch.setattr(_lib, "init", lambda: None)
    counts = check("tiny", precision, line_tile, fuse, padding_mode)
    r = row(precision, line_tile, fuse, padding_mode)
    assert counts == ROWS[r] and sum(counts.values()) == STEPS[r]


def test_hifigan_plan_table_v1(monkeypatch):
    """The published V1 generator (its 64- and 32-channel stages are the last two, the tiny one's the first two): the default network."""
    monkeypatch.setattr(_lib, "init", lambda: None)
    counts = check("v1", "f32", True, True, "zeros")
    assert counts == ROWS["f32 fused"] and sum(counts.values()) == STEPS["f32 fused"]


def rnd(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64) * 0.1


@pytest.mark.parametrize("split", [False, True])
def test_select_conv1d(split):
    """One accepted and one rejected geometry per kernel, on maps without storage."""
    M = lambda c: G.Map1D(1, 100, c, 32, split=split)
    pick = lambda c, k, role, **kw: G.select_conv1d(M(c), M(c), rnd(c, c, k), rnd(c), role=role, line_tile=True, split_tile=True, **kw)
    assert type(pick(128, 3, "conv1")) is G.GemmPlan and pick(128, 3, "conv1").kind == "gemm"                # 128 channels
    if split:
        assert type(pick(64, 3, "conv2", slope2=0.1)) is G.GemmPlan                                           # second convolutions from k = 7
        for p in (pick(64, 3, "conv1", act="leaky", slope=0.1), pick(64, 7, "conv2", dilation=1, slope2=0.1)):
            assert type(p) is G.TapsPlan and p.kind == "taps_x3" and p.split
        assert type(pick(32, 7, "conv1")) is G.GemmPlan                                                       # 64 channels only
        with pytest.raises(RuntimeError):                                                                      # no in-buffer activation
            pick(64, 7, "conv1", pre_slope=0.1)
    else:
        for p in (pick(64, 3, "conv2", slope2=0.1), pick(32, 11, "conv1", dilation=5, pre_slope=0.1)):
            assert type(p) is G.TapsPlan and p.kind == "taps" and not p.split
        assert pick(32, 11, "conv1", dilation=5, pre_slope=0.1).desc.pre_act == 1
    off = G.select_conv1d(M(64), M(64), rnd(64, 64, 7), rnd(64), role="conv1", line_tile=False, split_tile=False, dilation=3)
    assert type(off) is G.GemmPlan
    with pytest.raises(RuntimeError):
        G.select_conv1d(M(64), M(64), rnd(64, 64, 7), rnd(64), role="conv1", line_tile=False, split_tile=False, pre_slope=0.1)


@pytest.mark.parametrize("split", [False, True])
def test_select_resblock_step(split):
    M = lambda c: G.Map1D(1, 100, c, 32, split=split)
    pick = lambda c, k, fused=True, dil=1: G.select_resblock_step(M(c), M(c), rnd(c, c, k), rnd(c), rnd(c, c, k), rnd(c), dilation=dil,
                                                                   slope=0.1, fused=fused)
    p = pick(32, 11, dil=5)
    assert type(p).__name__ == ("ResblockPairX3Plan" if split else "ResblockPairPlan")
    assert p.kind == ("resblock_pair_x3" if split else "resblock_pair") and (p.desc.k, p.desc.dil) == (11, 5)
    assert pick(32, 11, fused=False) is None
    assert pick(64, 11) is None                              # fp16: two 90 KB weight tensors do not fit in LDS; split: 32 channels only
    if split:
        assert pick(64, 3) is None
    else:
        assert type(pick(64, 7, dil=5)) is G.ResblockPairPlan
