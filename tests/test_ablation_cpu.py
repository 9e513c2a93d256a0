"""CPU-only: the perturbation attributions (Occlusion, FeatureAblation): the kernels' closed forms and summation order against
the Captum-style restatement of tests/ablation_ref.py, argument checking in the engine and the captum.attr front end before
any GPU work, the error contract of the entry points of csrc/attribution_ablation.hip, and its resource usage."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import ablation_ref as R
from addvisor_hip import _lib, attribution as AT
from test_build_resources import resources


def shapes():
    """(L, win, stride) covering L - win divisible by stride and not, win == L, stride == win, stride 1."""
    out = [(100, 100, 1), (100, 100, 7), (100, 100, 100), (100, 10, 10), (100, 10, 3), (101, 10, 3), (100, 1, 1), (37, 5, 5),
           (37, 36, 2), (1600, 1600, 800), (16000, 1600, 800), (16003, 1600, 800), (5, 3, 1), (8, 8, 1), (9, 4, 4)]
    rng = np.random.default_rng(0)
    for _ in range(40):
        L = int(rng.integers(1, 300))
        win = int(rng.integers(1, L + 1))
        out.append((L, win, int(rng.integers(1, win + 1))))
    return out


def kernel_range(L, win, stride, K):
    """advh_ablation_accumulate's closed form: windows k_lo .. k_hi cover sample t."""
    t = np.arange(L)
    k_lo = np.where(t < win, 0, (t - win + stride) // stride)
    k_hi = np.minimum(K - 1, t // stride)
    return k_lo, k_hi


@pytest.mark.parametrize("L,win,stride", shapes())
def test_closed_form_windows_equal_the_padded_masks(L, win, stride):
    masks = R.occlusion_masks(L, win, stride)[:, 0].numpy()
    K = AT.occlusion_windows(L, win, stride)
    assert K == masks.shape[0] == AT.check_occlusion_args(L, win, stride)[2]
    assert masks.shape[1] == L                                  # the negative right pad crops the last window to L
    for k in range(K):                                          # window k covers [k * stride, min(k * stride + win, L))
        assert np.array_equal(np.flatnonzero(masks[k]), np.arange(k * stride, min(k * stride + win, L)))
    k_lo, k_hi = kernel_range(L, win, stride, K)
    assert np.all(k_lo <= k_hi)                                 # every sample is covered: no division by zero
    covered = np.arange(K)[:, None]
    want = (covered >= k_lo[None]) & (covered <= k_hi[None])
    assert np.array_equal(want, masks > 0)
    assert np.array_equal(k_hi - k_lo + 1, masks.sum(0).astype(np.int64))


def occlusion_kernel_model(f0, fk, L, win, stride):
    """numpy model of ablation_accumulate_kernel, Occlusion: float32 sum in increasing k from 0, then one rounded division."""
    B = f0.shape[0]
    K = fk.shape[0] // B
    k_lo, k_hi = kernel_range(L, win, stride, K)
    out = np.empty((B, L), np.float32)
    for b in range(B):
        d = (f0[b] - fk.reshape(K, B)[:, b]).astype(np.float32)
        for t in range(L):
            acc = np.float32(0)
            for k in range(k_lo[t], k_hi[t] + 1):
                acc = np.float32(acc + d[k])
            out[b, t] = np.float32(acc / np.float32(k_hi[t] - k_lo[t] + 1))
    return out


@pytest.mark.parametrize("L,win,stride", [(100, 10, 3), (101, 10, 1), (64, 64, 5), (50, 7, 7), (333, 40, 13)])
def test_kernel_summation_order_matches_captum_bit_for_bit(L, win, stride):
    B = 3
    K = AT.occlusion_windows(L, win, stride)
    g = torch.Generator().manual_seed(L + win)
    f0 = torch.randn(B, generator=g)
    fk = f0.repeat(K) + 1e-3 * torch.randn(K * B, generator=g) * torch.logspace(0, 3, K * B)   # diffs over three decades
    x = torch.randn(B, L, generator=g)
    ref, Kr = R.occlusion(x, 0.0, win, stride, f0=f0, fk=fk)
    assert Kr == K
    ours = occlusion_kernel_model(f0.numpy(), fk.numpy(), L, win, stride)
    assert np.array_equal(ours.view(np.int32), ref.numpy().view(np.int32))


def test_feature_gather_model_matches_captum():
    """FeatureAblation: attr[b, t] = diff[rank(id(b, t)), b] with the ranks of feature_indices equals the restatement's
    [min, max] loop, including ids absent from the mask and negative ids."""
    B, L = 3, 50
    g = torch.Generator().manual_seed(1)
    mask = torch.tensor([-4, 0, 3, 9])[torch.randint(0, 4, (B, L), generator=g)]
    index, K = AT.feature_indices(mask, B, L)
    assert K == 4 and index.dtype == torch.int32 and index.shape == (B, L)
    Kr = 9 - (-4) + 1
    f0 = torch.randn(B, generator=g)
    fk = torch.randn(Kr * B, generator=g)
    ref, _ = R.feature_ablation(torch.zeros(B, L), 0.0, mask, f0=f0, fk=fk)
    present = torch.tensor([-4, 0, 3, 9]) - (-4)
    fk_present = fk.view(Kr, B)[present]                                   # the engine evaluates the present ids only
    ours = f0[:, None] - fk_present[index.long(), torch.arange(B)[:, None]]
    assert torch.equal(ours, ref)
    idx, K = AT.feature_indices(None, B, L)
    assert K == L and torch.equal(idx, torch.arange(L, dtype=torch.int32)[None])
    idx, K = AT.feature_indices(torch.tensor([[5, 5, 6, 7, 6]], dtype=torch.uint8), B, 5)
    assert K == 3 and idx.tolist() == [[0, 0, 1, 2, 1]]


def test_ablated_batch_order():
    """The restatement's ablated rows are perturbation-major and keep x outside the window."""
    x = torch.arange(12, dtype=torch.float32).view(2, 6) + 1
    rows = R.ablated_batch(x, torch.full((1, 6), -1.0), R.occlusion_masks(6, 3, 2))
    assert rows.shape == (3 * 2, 6)
    assert rows[0].tolist() == [-1, -1, -1, 4, 5, 6] and rows[1].tolist() == [-1, -1, -1, 10, 11, 12]
    assert rows[5].tolist() == [7, 8, 9, 10, -1, -1]                       # k = 2, b = 1: the window cropped at L


def test_argument_helpers_raise_value_error():
    L = 100
    for window, stride in ((0, 1), (101, 1), (10, 11), ((10, 2), 1), (10, (1, 1)), (10, 0), (2.5, 1), (True, 1), (10, -1)):
        with pytest.raises(ValueError):
            AT.check_occlusion_args(L, window, stride)
    assert AT.check_occlusion_args(L, (10,), None) == (10, 1, 91)
    assert AT.check_occlusion_args(L, 100, 500) == (100, 500, 1)          # stride > win is allowed when win == L
    assert AT.check_occlusion_args(16000, 1600, 800)[2] == AT.occlusion_windows(16000, 1600, 800) == 19
    assert AT.occlusion_windows(64000, 1600, 800) == 79
    B = 2
    for bad in (torch.zeros(B, L), torch.zeros(B, L, dtype=torch.bool), torch.zeros(3, L, dtype=torch.int64),
                torch.zeros(B, L - 1, dtype=torch.int64), torch.zeros(L, dtype=torch.int64), np.zeros((B, L), np.int64),
                torch.tensor([[-2 ** 30, 2 ** 30] + [0] * (L - 2)])):
        with pytest.raises(ValueError):
            AT.feature_indices(bad, B, L)
    assert AT.feature_indices(torch.tensor([[-2 ** 30, 2 ** 30 - 1] + [0] * (L - 2)]), B, L)[1] == 3   # id - id_min fits in int32
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            AT.check_internal_batch(bad)
    assert AT.check_internal_batch(None) == 128


def test_engine_validates_before_gpu_work():
    """Argument errors surface before the engine touches the device (the engine object is never used)."""
    att = AT.HipAttribution.__new__(AT.HipAttribution)
    x = torch.zeros(2, 100)
    for call in (lambda: att.occlusion(x, 101), lambda: att.occlusion(x, 10, 11), lambda: att.occlusion(x, 10, baselines=torch.zeros(3, 100)),
                 lambda: att.occlusion(x, 10, internal_batch_size=0), lambda: att.occlusion(torch.zeros(2, 3, 4), 2),
                 lambda: att.feature_ablation(x, feature_mask=torch.zeros(2, 100)),
                 lambda: att.feature_ablation(x, feature_mask=torch.zeros(1, 99, dtype=torch.int64)),
                 lambda: att.feature_ablation(x, baselines=torch.zeros(2, 99))):
        with pytest.raises(ValueError):
            call()


class _NoEngine:
    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import FeatureAblation, Occlusion
    x = torch.zeros(2, 100)
    occ, fa = Occlusion(_NoEngine()), FeatureAblation(_NoEngine())
    for call in (lambda: occ.attribute(x, (10,), target=0), lambda: occ.attribute(x, (101,)), lambda: occ.attribute(x, (10,), strides=(11,)),
                 lambda: occ.attribute(x, (10,), baselines=torch.zeros(2, 99)), lambda: occ.attribute(x, (10,), perturbations_per_eval=0),
                 lambda: occ.attribute(x[0], (10,)), lambda: fa.attribute(x, target=1),
                 lambda: fa.attribute(x, feature_mask=torch.zeros(2, 100)), lambda: fa.attribute(x, perturbations_per_eval=1.5),
                 lambda: fa.attribute(x, baselines=torch.zeros(3, 100))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(AssertionError):                          # valid arguments go on to the engine
        occ.attribute(x, (10,), strides=(5,))


def test_captum_names_and_signatures():
    from captum.attr import FeatureAblation, Occlusion
    import captum_saliency
    assert captum_saliency.Occlusion is Occlusion and captum_saliency.FeatureAblation is FeatureAblation
    p = inspect.signature(Occlusion.attribute).parameters
    assert list(p) == ["self", "inputs", "sliding_window_shapes", "strides", "baselines", "target", "additional_forward_args",
                       "perturbations_per_eval", "show_progress"]
    assert (p["strides"].default, p["baselines"].default, p["perturbations_per_eval"].default, p["show_progress"].default) == (None, None, 1, False)
    p = inspect.signature(FeatureAblation.attribute).parameters
    assert list(p) == ["self", "inputs", "baselines", "target", "additional_forward_args", "feature_mask", "perturbations_per_eval",
                       "show_progress"]
    assert (p["feature_mask"].default, p["perturbations_per_eval"].default) == (None, 1)
    p = inspect.signature(captum_saliency.explain_waves).parameters
    assert (p["method"].default, p["window"].default, p["stride"].default) == ("input_x_gradient", 1600, 800)


def test_argument_errors_of_the_ablation_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched) for the perturbation entry points: validation
    happens before any HIP call, so it runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ib = (C.c_int32 * 64)()
    pi = C.addressof(ib)

    def desc(**kw):
        d = dict(x=p, base=p, mask=None, n=8, B=2, base_rows=1, mask_rows=0, mode=0, win=4, stride=2, K=3)
        d.update(kw)
        return AT.AblationDesc(**d)

    pts = lambda d, row0=0, rows=6, out=p: lib.advh_ablation_points(C.byref(d) if d else None, row0, rows, out, None)
    acc = lambda d, f0=p, fk=p, attr=p: lib.advh_ablation_accumulate(C.byref(d) if d else None, f0, fk, attr, None)
    feat = desc(mode=1, mask=pi, mask_rows=2, win=0, stride=0, K=5)
    assert pts(None) == EINVAL and acc(None) == EINVAL
    for bad in (desc(x=None), desc(base=None), desc(B=0), desc(n=0), desc(K=0), desc(base_rows=0), desc(base_rows=3),
                desc(win=0), desc(stride=0), desc(stride=-1), desc(win=9), desc(win=2, stride=3, K=4),   # stride > win < n
                desc(K=4), desc(mode=2), desc(mode=-1), desc(mode=1, mask=None, mask_rows=1, K=2), desc(mode=1, mask=pi, mask_rows=0, K=2),
                desc(mode=1, mask=pi, mask_rows=3, K=2)):
        assert pts(bad) == EINVAL, bad
        assert acc(bad) == EINVAL, bad
    assert pts(desc(), rows=-1) == EINVAL and pts(desc(), row0=-1) == EINVAL and pts(desc(), out=None) == EINVAL
    assert pts(feat, out=None) == EINVAL
    assert acc(desc(), f0=None) == EINVAL and acc(desc(), fk=None) == EINVAL and acc(feat, attr=None) == EINVAL
    assert pts(desc(), rows=0) == 0                                        # nothing to write: no launch
    assert pts(desc(win=8, stride=50, K=1), rows=0) == 0                   # stride > win is allowed when win == n


def test_ablation_kernels_do_not_spill():
    res = resources("attribution_ablation.hip")
    for nm, forms in (("build_rows_kernel", 2), ("ablation_accumulate_kernel", 1)):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == forms, (nm, sorted(res))                       # float4 and scalar forms of the points kernel
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
