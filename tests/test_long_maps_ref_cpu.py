"""CPU-only: the yardsticks of tests/test_gpu_long_maps.py beyond 256 frames.  ``attention_rollout_ref.explain`` and
``lrp_ref.explain`` evaluated in float32 stay within 1e-5 of each tensor's max|float64 result| at 299 and 513 frames on the tiny
post-LN and pre-LN models -- a tenth of the engine's f32 bar, as tests/test_attention_rollout_cpu.py and tests/test_lrp_cpu.py
show up to 249 frames -- so the bar measures the engine and not the restatements' conditioning at these lengths.  Also the numpy
fp32 restatement of the streamed (m, 1/l) recurrences in blocks of 128 (tests/attention_maps_long_cases.py), against float64 and
against its own one-block form; tests/test_build_resources_attention_maps_long.py holds its row sums on the kernel suite's inputs."""
import math

import numpy as np
import pytest
import torch

import attention_maps_long_cases as M
import attention_rollout_ref as AR
import backward_ops_ref as BR
import lrp_ref as LR
from addvisor_hip import synthetic as syn

LENGTHS = {96000: 299, 164240: 513}
MODELS = {"post_ln": lambda: syn.tiny_config(False), "pre_ln": lambda: syn.tiny_config(True)}
BAR = 1e-5


def model_of(name):
    cfg = MODELS[name]()
    return (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))


def rel(a, b):
    return ((a.double() - b).abs().max() / (b.abs().max() + 1e-300)).item()


@pytest.mark.parametrize("L", list(LENGTHS))
@pytest.mark.parametrize("name", list(MODELS))
def test_float32_restatements_stay_a_tenth_of_the_bar_from_float64(name, L):
    mdl = model_of(name)
    x = syn.make_clips(1, L, seed=91)
    worst = {}
    with torch.enable_grad():
        a64, a32 = AR.explain(x, mdl), AR.explain(x, mdl, dtype=torch.float32)
        l64, l32 = LR.explain(x, mdl), LR.explain(x, mdl, dtype=torch.float32)
        i64, i32 = LR.explain(x, mdl, gelu_rule="identity"), LR.explain(x, mdl, gelu_rule="identity", dtype=torch.float32)
    assert a64["A"][0].shape[-1] == LENGTHS[L]
    for l in range(len(a64["A"])):
        worst[f"A[{l}]"] = rel(a32["A"][l], a64["A"][l])
        worst[f"Abar[{l}]"] = rel(a32["Abar"][l], a64["Abar"][l])
    for f in AR.FUSIONS:
        worst[f"R {f}"], worst[f"rel {f}"] = rel(a32["R"][f], a64["R"][f]), rel(a32["rel"][f], a64["rel"][f])
    worst["D"], worst["rel_grad"] = rel(a32["D"], a64["D"]), rel(a32["rel_grad"], a64["rel_grad"])
    for tag, (r32, r64) in (("lrp", (l32, l64)), ("lrp identity", (i32, i64))):
        worst[f"{tag} R"], worst[f"{tag} rel"] = rel(r32["R"], r64["R"]), rel(r32["rel"], r64["rel"])
    print(f"{name} L={L} ({LENGTHS[L]} frames): float32 vs float64, of max|ref|: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) < BAR, {k: v for k, v in worst.items() if v >= BAR}


@pytest.mark.parametrize("T", [1, 17, 128, 129, 273, 513])
def test_streamed_statistics_restatement(T):
    """Blocks of 128 with a running maximum and a rescaled running sum: against float64 softmax, and m equal to the one-block
    form's bit for bit (a maximum does not depend on the blocking)."""
    heads, dm, B = 3, 40, 2
    g = torch.Generator().manual_seed(T)
    qkv = (torch.randn(B * T, 3 * heads * dm, generator=g) * 0.7).half().double()
    m, inv, P = M.stats_np32(qkv, B, T, heads, dm)
    m1, inv1, P1 = M.stats_np32(qkv, B, T, heads, dm, block=1 << 20)
    q, k, _ = BR.heads_of(qkv, B, T, heads, dm)
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dm), -1).numpy()
    e, e1, dev = np.abs(P - ref).max() / ref.max(), np.abs(P1 - ref).max() / ref.max(), M.rowsum_deviation(P)
    print(f"T={T}: streamed {e:.2e}, one block {e1:.2e} of max|ref|; rows sum to 1 within {dev:.2e}")
    assert np.array_equal(m, m1) and e < 0.5 * M.TOL_MAPS and e1 < 0.5 * M.TOL_MAPS and dev <= M.ROWSUM_NP32_WORST
    assert P.dtype == np.float32 and m.dtype == np.float32 and inv.dtype == np.float32
