"""CPU-only: which kernel every layer of the inference U-Net gets (``gemm.select_conv2d`` / ``gemm.select_upconv2d``), for all eight
combinations of precision x line_tile x fuse_up at 1 x 512 x 196.  ``HipUNet._workspace`` plans on the CPU once ``_lib.init`` is stubbed:
plans are host objects until ``run``."""
import pytest
import torch

from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.unet import HipUNet

ENCODER = ["x1", "x2a", "x2", "x3a", "x3", "x4a", "x4", "b1", "b2"]
UNFUSED = ENCODER + ["u4", "y4a", "y4", "u3", "y3a", "y3", "u2", "y2a", "y2", "u1", "y1a", "y1"]
FUSED = ENCODER + ["y4a", "y4", "y3a", "y3", "y2a", "y2", "y1a", "y1"]
TAPS2D = {"f16": "Taps2dPlan", "f32": "Taps2dSplitPlan"}
CONV_S21 = {"f16": "ConvS21TilePlan", "f32": "ConvS21SplitTilePlan"}
UPCONV = {"f16": "UpconvTilePlan", "f32": "UpconvSplitTilePlan"}


def expected(precision, line_tile, fuse_up):
    """{destination map: plan class} of the layers that are not a plain ``GemmPlan``."""
    table = {}
    if fuse_up:
        table.update(y4a="PlanGroup", y3a="PlanGroup", y2a="PlanGroup", y1a="PlanGroup")
    if line_tile:
        table.update({dst: TAPS2D[precision] for dst in ("x1", "x2", "y2", "y1")})
        if fuse_up:                                            # e2.block.0's tile: on the fused network only
            table.update(x2a=CONV_S21[precision], y1a=UPCONV[precision])
    return table


@pytest.mark.parametrize("fuse_up", [False, True])
@pytest.mark.parametrize("line_tile", [False, True])
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_unet_plan_table(monkeypatch, precision, line_tile, fuse_up):
    monkeypatch.setattr(_lib, "init", lambda: None)
    net = HipUNet(syn.unet_weights(), torch.device("cpu"), line_tile=line_tile, fuse_up=fuse_up, precision=precision)
    ws = net._workspace(1, 512, 196)
    steps = ws["steps"]
    assert len(steps) == (17 if fuse_up else 21)
    assert [dst for _, _, dst in steps] == (FUSED if fuse_up else UNFUSED)
    table = expected(precision, line_tile, fuse_up)
    assert [type(p).__name__ for p, _, _ in steps] == [table.get(dst, "GemmPlan") for _, _, dst in steps]
    heads = [getattr(p, "head", None) is not None for p, _, _ in steps]
    if precision == "f32" and line_tile:
        assert heads == [False] * (len(steps) - 1) + [True]
        assert ws["maps"]["y1"].t is None
    else:
        assert not any(heads)
        assert ws["maps"]["y1"].t is not None
    assert ("xin" in ws["maps"]) == fuse_up and ("u1" in ws["maps"]) == (not fuse_up)


def rnd(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64) * 0.1


@pytest.mark.parametrize("split", [False, True])
def test_select_conv2d(split):
    """One accepted and one rejected geometry per kernel, on maps without storage."""
    F = lambda h, w, c, ph=1, pw=1: G.FMap(1, h, w, c, ph, pw, split=split)
    kinds = ("taps2d_x3", "conv53s21_x3") if split else ("taps2d", "conv53s21")
    pick = lambda *a, **k: G.select_conv2d(*a, line_tile=True, **k)
    p = pick([F(16, 12, 64)], F(16, 12, 64), rnd(64, 64, 3, 3), rnd(64))
    assert p.kind == kinds[0] and type(p).__name__ == ("Taps2dSplitPlan" if split else "Taps2dPlan")
    assert type(pick([F(16, 12, 128)], F(16, 12, 128), rnd(128, 128, 3, 3), rnd(128))) is G.GemmPlan        # 128 channels
    e2 = dict(stride=(2, 1), padding=(2, 1))
    p = pick([F(16, 12, 32, 2, 1)], F(8, 12, 64), rnd(64, 32, 5, 3), rnd(64), **e2)
    assert p.kind == kinds[1] and type(p).__name__ == ("ConvS21SplitTilePlan" if split else "ConvS21TilePlan")
    g = pick([F(16, 12, 32, 2, 1)], F(8, 12, 64), rnd(64, 32, 5, 3), rnd(64), s21_tile=False, **e2)
    assert type(g) is G.GemmPlan and g.desc.M == 8 * 12 and not g.desc.halo_zero                              # interior rows only
    assert type(pick([F(16, 12, 32)], F(8, 12, 64), rnd(64, 32, 3, 3), rnd(64), stride=(2, 1))) is G.GemmPlan   # a 3 x 3 kernel
    g = G.select_conv2d([F(16, 12, 64)], F(16, 12, 64), rnd(64, 64, 3, 3), rnd(64), line_tile=False, interior_only=False)
    assert type(g) is G.GemmPlan and g.desc.M == 18 * 14 and g.desc.halo_zero


@pytest.mark.parametrize("split", [False, True])
def test_select_upconv2d(split):
    F = lambda h, w, c: G.FMap(1, h, w, c, 1, 1, split=split)
    d1 = (F(8, 12, 64), F(16, 12, 8), F(16, 12, 32), rnd(64, 32, 2, 1), rnd(32), rnd(32, 33, 3, 3), rnd(32))
    d1_kw = dict(stride=(2, 1), coarse_C=64, skip_C=1, indicator=("skip", 1))
    p = G.select_upconv2d(*d1, line_tile=True, **d1_kw)
    assert p.kind == ("upconv21_x3" if split else "upconv21") and type(p).__name__ == ("UpconvSplitTilePlan" if split else "UpconvTilePlan")
    assert type(G.select_upconv2d(*d1, line_tile=False, **d1_kw)) is G.PlanGroup
    d2 = (F(8, 12, 192), F(16, 12, 32), F(16, 12, 64), rnd(128, 64, 2, 1), rnd(64), rnd(64, 96, 3, 3), rnd(64))      # up2 + d2.block.0
    assert type(G.select_upconv2d(*d2, line_tile=True, stride=(2, 1), coarse_C=128, skip_C=32, indicator=("coarse", 128))) is G.PlanGroup
