#!/usr/bin/env python3
"""Mask-domain IntegratedGradients (HipSpectralAttribution) next to the waveform IntegratedGradients over the same clips, in one
process: wav2vec2-base shape, fp32-class chain, 16 clips x 4 s, 50 Gauss-Legendre steps (800 path points, 128 per chunk), a
non-zero baseline for both (a random mask / a noise clip, so that both run the baseline-aware path of
csrc/attribution_paths.hip).  Measured, alternated, each the median of 3 timed calls after one warm-up of each:
  - ``mask_ig``: HipSpectralAttribution.integrated_gradients over the full (513, T) mask -- per chunk the path points with
    n = 513 T, advh_istft_masked_rows, the whole chain forward and backward, advh_istft_masked_rows_bwd, the accumulate;
  - ``wave_ig``: HipAttribution.integrated_gradients over the same number of path points;
  - ``rows_launches``: the two row-mapped STFT-class launches alone over the same rows (one forward and one adjoint launch per
    chunk of 128 rows).
The tool's one condition (exit status 1 otherwise): a mask-domain path point costs no more than a waveform path point plus
the stand-alone time of the two launches per row, plus 10 % of that sum (the launch gaps and the larger accumulate rows:
513 T = 102 087 floats per row against 64 000).  Times come from device events."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import ops, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402
from addvisor_hip.spectral_attribution import HipSpectralAttribution  # noqa: E402

torch.set_grad_enabled(False)
B, L, STEPS, REPS, CHUNK = 16, 64000, 50, 3, 128
if not torch.cuda.is_available():
    sys.exit("bench_spectral_attr.py measures on a GPU; none is available")
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
w = syn.make_clips(B, L).to(dev)
eng = HipSpectralAttribution(att, w, "linear")
T = eng.T
gen = torch.Generator().manual_seed(3)
wave_base = (0.05 * torch.randn(B, L, generator=gen)).to(dev)
mask = torch.ones(B, 513, T, device=dev)
mask_base = torch.rand(B, 513, T, generator=gen).to(dev)
rows = torch.rand(CHUNK, 513, T, generator=gen).to(dev)
g_wave = torch.randn(CHUNK, L, generator=gen).to(dev)
points = B * STEPS
nchunk = -(-points // CHUNK)


def rows_launches():
    for c in range(nchunk):
        ops.istft_masked_rows(eng.spec, rows, L, "linear", row0=c * CHUNK)
        ops.istft_masked_rows_bwd(g_wave, eng.spec, rows, "linear", row0=c * CHUNK)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


methods = {"mask_ig": lambda: eng.integrated_gradients(mask, n_steps=STEPS, baselines=mask_base, internal_batch_size=CHUNK),
           "wave_ig": lambda: att.integrated_gradients(w, n_steps=STEPS, baselines=wave_base, internal_batch_size=CHUNK),
           "rows_launches": rows_launches}
for fn in methods.values():
    once(fn)
ts = {k: [] for k in methods}
for _ in range(REPS):
    for k, fn in methods.items():
        ts[k].append(once(fn))
med = {k: statistics.median(v) for k, v in ts.items()}
per_row = {"mask_ig": med["mask_ig"] / points, "wave_ig": med["wave_ig"] / points, "rows_launches": med["rows_launches"] / (nchunk * CHUNK)}
out = {"workload": f"wav2vec2-base shape, fp32-class chain, {B} clips x 4 s, {STEPS} steps ({points} path points, {CHUNK} per chunk), "
                   f"mask (513, {T}), linear domain"}
for k in methods:
    out[k] = {"s_per_call": round(med[k], 4), "ms_per_row": round(1e3 * per_row[k], 4),
              "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4)}
out["mask_ig"]["path_points_per_s"] = round(points / med["mask_ig"], 1)
out["wave_ig"]["path_points_per_s"] = round(points / med["wave_ig"], 1)
bound = 1.10 * (per_row["wave_ig"] + per_row["rows_launches"])
out["bound_ms_per_row"] = round(1e3 * bound, 4)
out["mask_over_wave"] = round(per_row["mask_ig"] / per_row["wave_ig"], 4)
out["within_bound"] = per_row["mask_ig"] <= bound
out["finite"] = bool(torch.isfinite(eng.integrated_gradients(mask, n_steps=4, baselines=mask_base)).all().item())
print(json.dumps(out))
sys.exit(0 if out["within_bound"] and out["finite"] else 1)
