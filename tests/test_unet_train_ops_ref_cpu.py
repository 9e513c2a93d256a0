"""Pins tests/unet_train_ops_ref.py (the fp64 restatements that tests/test_gpu_unet_train_kernels.py compares the U-Net training
kernels with) to torch's own fp64 operators, and checks on the CPU what the GPU file's tolerance bars rest on: the fp64
reference alone keeps the LeakyReLU band under its cap for every case's seed, and the fp32 ONE-pass BatchNorm exceeds the
bars of the offset kinds (so a kernel of that quality fails them).  Also: the case lists name every entry point."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_train_kernel_cases as K
import unet_train_ops_ref as R
from addvisor_hip import _lib

TOL = 1e-12


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def test_batchnorm_forward_and_running_buffers_equal_nn_batchnorm2d():
    g = torch.Generator().manual_seed(5)
    C, slope = 12, 0.2
    bn = torch.nn.BatchNorm2d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        bn.num_batches_tracked.fill_(41)
    rm, rv, nbt = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(), 41
    for step, (B, H, W) in enumerate([(2, 3, 5), (1, 1, 2)]):          # the second update has n = 2
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 3.0 + 7.0
        with torch.no_grad():
            want = F.leaky_relu(bn(x), slope)
        coef, var, y, act = R.bn_forward(_nhwc(x), bn.weight.detach().numpy(), bn.bias.detach().numpy(), 1e-5, slope)
        rm, rv, nbt = R.bn_running(rm, rv, nbt, coef[2], var, float(B * H * W), 0.1)
        assert rel(act, _nhwc(want)) <= TOL
        assert rel(coef[0] * _nhwc(x) + coef[1], y) <= TOL               # the scale / shift form the kernel applies
        assert rel(rm, bn.running_mean.numpy()) <= TOL and rel(rv, bn.running_var.numpy()) <= TOL
        assert nbt == int(bn.num_batches_tracked)


@torch.enable_grad()          # other test modules switch autograd off for the whole process
def test_batchnorm_backward_equals_autograd():
    g = torch.Generator().manual_seed(6)
    B, C, H, W, slope, inv_scale = 2, 8, 3, 5, 0.2, 1.0 / 64
    x = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2.0 + 3.0).requires_grad_()
    gamma = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    gout = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    y = F.leaky_relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, 1e-5), slope)
    y.backward(gout * 64.0)                                            # the kernels see the loss-scaled gradient
    coef, _, _, _ = R.bn_forward(_nhwc(x.detach()), gamma.detach().numpy(), beta.detach().numpy(), 1e-5, slope)
    r = R.bn_backward(_nhwc(x.detach()), _nhwc(gout * 64.0), coef, slope, inv_scale)
    assert rel(r["dz"], _nhwc(x.grad)) <= TOL                          # dz stays scaled, the affine gradients are unscaled
    assert rel(r["dgamma"], gamma.grad.numpy() / 64.0) <= TOL and rel(r["dbeta"], beta.grad.numpy() / 64.0) <= TOL
    n = B * H * W
    assert rel(r["coef_b"][1] * n, r["sums"][0]) <= TOL and rel(r["coef_b"][2] * n, r["sums"][1]) <= TOL
    assert np.array_equal(r["coef_b"][0], coef[0])


def test_stem_and_weight_gradients_equal_torch():
    g = torch.Generator().manual_seed(7)
    B, H, W, Fq, Tq = 2, 6, 7, 9, 8
    mag = torch.randn(B, Fq, Tq, generator=g, dtype=torch.float64)
    x = mag[:, :H, :W].unsqueeze(1)
    w = torch.randn(32, 1, 5, 3, generator=g, dtype=torch.float64)
    b = torch.randn(32, generator=g, dtype=torch.float64)
    want = F.leaky_relu(F.conv2d(x, w, b, stride=(2, 1), padding=(2, 1)), 0.2)
    assert rel(R.stem(mag.numpy(), H, W, w.numpy().reshape(32, 15), b.numpy(), 0.2), _nhwc(want)) <= TOL
    dz = torch.randn(B, 32, H // 2, W, generator=g, dtype=torch.float64)
    want = torch.nn.grad.conv2d_weight(x, w.shape, dz, stride=(2, 1), padding=(2, 1))
    assert rel(R.stem_wgrad(_nhwc(dz), mag.numpy(), H, W), want.numpy().reshape(32, 15)) <= TOL
    dz = torch.randn(B, 32, H, W, generator=g, dtype=torch.float64)
    want = torch.nn.grad.conv2d_weight(x, (32, 1, 3, 3), dz, padding=1)
    assert rel(R.skip_wgrad(_nhwc(dz), mag.numpy(), H, W), want.numpy().reshape(32, 9)) <= TOL


@torch.enable_grad()          # other test modules switch autograd off for the whole process
def test_head_equals_autograd():
    g = torch.Generator().manual_seed(8)
    y = torch.randn(2, 3, 5, 32, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(32, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn((), generator=g, dtype=torch.float64).requires_grad_()
    dmask = torch.randn(2, 3, 5, generator=g, dtype=torch.float64)
    m = torch.sigmoid(y @ w + b)
    m.backward(dmask)
    mask, logits = R.head(y.detach().numpy(), w.detach().numpy(), float(b.detach()))
    assert rel(mask, m.detach().numpy()) <= TOL
    dlogit, dy1 = R.head_bwd(dmask.numpy(), mask, w.detach().numpy(), 64.0)
    assert rel(dy1 / 64.0, y.grad.numpy().reshape(-1, 32)) <= TOL
    assert rel(R.head_wgrad(dlogit, y.detach().numpy()), np.concatenate([w.grad.numpy(), [float(b.grad)]])) <= TOL


def test_transpose_gather_equals_unfold():
    """3x3 taps, stride 1: the index map is im2col of the zero-padded interior."""
    rng = np.random.default_rng(9)
    B, H, W, Cc = 2, 4, 5, 8
    src = rng.standard_normal((B, H + 2, W + 2, Cc))
    src[:, 0] = src[:, -1] = 55.0
    src[:, :, 0] = src[:, :, -1] = 55.0                                 # a halo that must not be read
    d = K.tr_desc(B, H, W, 0, 0, H, W, 1, 1, Cc, 0, Cc, 1, 1, [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)])
    out = R.transpose_gather(src, d, np.full((9 * Cc, d["ld"]), -1.0))
    x = torch.from_numpy(R.interior(src, 1, 1)).permute(0, 3, 1, 2)
    cols = F.unfold(x, 3, padding=1).reshape(B, Cc, 9, H * W).permute(2, 1, 0, 3).reshape(9 * Cc, B * H * W)
    assert np.array_equal(out[:, :B * H * W], cols.numpy()) and (out[:, B * H * W:] == -1.0).all()


def test_pack_x_and_split_round():
    rng = np.random.default_rng(10)
    mag = rng.standard_normal((2, 5, 4))
    cat = np.full((2, 3 + 4, 2 + 2, 40), 7.0)
    out = R.pack_x(mag, 3, 2, cat, 32, 2, 1)
    it = R.interior(out, 2, 1)
    assert np.array_equal(it[..., 32], mag[:, :3, :2]) and (it[..., 33] == 1).all() and (it[..., 34:] == 0).all() and (it[..., :32] == 7).all()
    keep = np.ones(out.shape, bool)
    R.interior(keep, 2, 1)[...] = False
    assert (out[keep] == 7.0).all()
    x = torch.randn(4096, dtype=torch.float64) * 100.0
    from addvisor_hip import gemm as G
    a, b = R.split_round(x.numpy()), G.join_planes(G.split_planes(x)).double().numpy()
    # the host packer converts fp64 -> fp16 through fp32: a value within an fp32 ulp of an fp16 tie lands one lo-ulp away
    assert (a != b).mean() <= 1e-3 and (np.abs(a - b) <= 2.0 ** -21 * np.abs(b)).all()


@pytest.mark.parametrize("case", K.BN_FWD_CASES, ids=K.case_id)
def test_forward_bars_are_sharp_and_the_band_stays_under_its_cap(case):
    d = K.bn_fwd_data(case)
    assert d["band"].mean() <= K.BAND_CAP
    bars, e2 = K.bn_fwd_bars(d)
    assert (d["var"][3::4] == 0).all() and (d["two"][1][3::4] == 0).all()        # constant channels: variance exactly 0
    if d["n"] < 30:
        return
    coef1, _, act1 = R.bn_forward_f32_one_pass(d["zi"], d["gamma"], d["beta"], K.EPS, K.SLOPE)
    e1 = K.bn_fwd_errors(d, coef1.astype(np.float64), K.quant(act1, d["fmt"]))
    for k in (1, 2):                                                             # mu = 8, mu = 64
        assert e1["invstd", k] > bars["invstd", k], (K.KINDS[k], e1["invstd", k], bars["invstd", k])
        assert e1["scale", k] > bars["scale", k]
    if d["fmt"] == "split":                                                      # an fp16 activation's own rounding (2^-11) hides it
        for k in (1, 2):
            assert e1["act", k] > bars["act", k], (K.KINDS[k], e1["act", k], bars["act", k])


@pytest.mark.parametrize("case", [c for c in K.BN_BWD_CASES if c[1] != "trip2"] + [c for c in K.BN_BWD_CASES if c[1] == "trip2"][:3], ids=K.case_id)
def test_backward_band_stays_under_its_cap_and_bars_stay_under_the_projects(case):
    d = K.bn_bwd_data(case)
    assert d["band"].mean() <= K.BAND_CAP
    ref, bars, e2 = K.bn_bwd_refs(d, d["y"] > 0)
    for (q, k), b in bars.items():                     # the fp32 restatement itself meets every bar: the bars are attainable in fp32
        assert b <= K.PROJECT_BAR[d["gfmt"]] * np.abs(ref[q]).max() and e2[q, k] <= b, (q, k, e2[q, k], b)


def test_case_lists_name_every_entry_point():
    names = [n for n in _lib.SIGNATURES if n.startswith(K.ENTRY_PATTERNS)]
    assert len(names) >= 26
    missing = [n for n in names if not K.ENTRY_CASES.get(n)]
    assert not missing, f"entry points without a case in tests/unet_train_kernel_cases.py: {missing}"
