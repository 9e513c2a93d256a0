#!/usr/bin/env python3
"""The per-clip optimised mask (HipSpectralAttribution.optimize_mask) next to the seeded gradient it is built around, in one
process: wav2vec2-base shape, fp32-class chain, 16 clips x 4 s, the full (513, T) mask, cell (16, 4), 50 Adam steps, all 32
rows (mask-in / mask-out per clip) in one chunk.  Measured, alternated, each the median of 3 timed calls after one warm-up of
each:
  - ``optimize_mask``: the whole call -- F(ones), per step rank, rows, ISTFT rows, forward, terms, backward(seed=), ISTFT
    adjoint, step, then the final check and the final forward of the mask and its complement;
  - ``seeded_gradient``: 50 times the seeded gradient alone over the same 32 rows (ISTFT rows, forward, backward(seed=), ISTFT
    adjoint), fixed rows and seeds;
  - ``launches``: 50 times the four non-chain launches alone (advh_feature_rank, advh_mask_opt_rows, advh_mask_opt_terms,
    advh_mask_opt_step) on fixed operands.
Reported: clip-steps per second, the ratio of the optimiser's step rate to the seeded gradient's (the aim is >= 0.95; an aim,
not a condition: the exit status only says that the result is finite), and the time of the four launches per step.  Times come
from device events."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import attribution as AT, mask_opt as MO, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402
from addvisor_hip.spectral_attribution import HipSpectralAttribution  # noqa: E402

torch.set_grad_enabled(False)
B, L, STEPS, REPS, CELL = 16, 64000, 50, 3, (16, 4)
if not torch.cuda.is_available():
    sys.exit("bench_mask_opt.py measures on a GPU; none is available")
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
eng = HipSpectralAttribution(att, syn.make_clips(B, L).to(dev), "linear")
T = eng.T
a = MO.check_mask_opt_args(B, T, "linear", steps=STEPS, cell=CELL, seed=1)
d, K, n = a.desc(), a.K, a.Fm * a.Tm
f32 = dict(dtype=torch.float32, device=dev)
theta = a.theta0.to(dev)
rows = MO.mask_rows(d, theta, 0, B)
gen = torch.Generator().manual_seed(3)
seeds = (0.5 * torch.randn(2 * B, generator=gen)).to(dev)
G = torch.randn(2 * B, n, generator=gen).to(dev)
logits = torch.randn(2 * B, generator=gen).to(dev)
sign = torch.ones(B, **f32)
p, hist, m1, m2, sd_out = torch.empty((B, K), **f32), torch.zeros((B, 6), **f32), torch.zeros((B, K), **f32), torch.zeros((B, K), **f32), \
    torch.empty(2 * B, **f32)
eng._rows.Fm, eng._rows.Tm = a.Fm, a.Tm


def seeded_gradient():
    for _ in range(STEPS):
        eng._rows._row_gradient_seeded(rows, lambda lg: seeds, 0, 1, 2)


def launches():
    th = theta.clone()
    for k in range(STEPS):
        rank = AT.feature_rank(th.view(B, K), False)
        MO.mask_rows(d, th, 0, B, rows)
        MO.mask_terms(d, th, rank, sign, logits, 0, B, p, sd_out, hist)
        MO.mask_step(d, th, p, rank, G, 0, B, k + 1, m1, m2, None)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


methods = {"optimize_mask": lambda: eng.optimize_mask(steps=STEPS, cell=CELL, seed=1), "seeded_gradient": seeded_gradient,
           "launches": launches}
for fn in methods.values():
    once(fn)
ts = {k: [] for k in methods}
for _ in range(REPS):
    for k, fn in methods.items():
        ts[k].append(once(fn))
med = {k: statistics.median(v) for k, v in ts.items()}
out = {"workload": f"wav2vec2-base shape, fp32-class chain, {B} clips x 4 s, mask (513, {T}), cell {CELL} (grid ({a.Fc}, {a.Tc})), "
                   f"{STEPS} Adam steps, {2 * B} rows per step, linear domain"}
for k in methods:
    out[k] = {"s_per_call": round(med[k], 4), "ms_per_step": round(1e3 * med[k] / STEPS, 4), "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4)}
out["clip_steps_per_s"] = round(B * STEPS / med["optimize_mask"], 1)
out["step_rate_over_seeded_gradient"] = round(med["seeded_gradient"] / med["optimize_mask"], 4)
out["aim_0.95_met"] = out["step_rate_over_seeded_gradient"] >= 0.95
res = eng.optimize_mask(steps=4, cell=CELL, seed=1)
out["finite"] = bool(torch.isfinite(res.mask).all().item())
out["area_reached_after_4_steps"] = [round(v, 4) for v in res.area_reached.tolist()]
print(json.dumps(out))
sys.exit(0 if out["finite"] else 1)
