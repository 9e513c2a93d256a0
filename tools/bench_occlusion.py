#!/usr/bin/env python3
"""Ablated rows per second of Occlusion next to the plain classifier forward over the same rows, in one process:
wav2vec2-base shape, fp32-class, 16 clips x 4 s, window 1600, stride 800 (K = 79 windows, 1 264 ablated rows), internal
batch 128.  The plain figure is ``emb.forward`` on the same number of 128-row chunks (the ablation's padded last chunk
included), so the ratio is what the points / accumulate kernels, the F(x) forward and the logit copies cost.  Times come from
device events around each call; each figure is the median of 7 timed runs after two warm-up calls."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import attribution as AT, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

torch.set_grad_enabled(False)
B, L, WIN, STRIDE, CHUNK, REPS = 16, 64000, 1600, 800, 128, 7
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32")
att = HipAttribution(emb)
w = syn.make_clips(B, L).to(dev)
K = AT.occlusion_windows(L, WIN, STRIDE)
rows = K * B
nchunk = -(-rows // CHUNK)
pts = syn.make_clips(CHUNK, L, seed=7).to(dev)


def plain():
    for _ in range(nchunk):
        emb.forward(pts, want_hidden=False)


def occlusion():
    return att.occlusion(w, WIN, STRIDE, internal_batch_size=CHUNK)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) / 1e3)
    return statistics.median(ts), ts


res = {}
for name, fn in (("plain_forward", plain), ("occlusion", occlusion), ("plain_forward_again", plain)):   # A-B-A
    med, ts = timed(fn)
    res[name] = {"s": round(med, 4), "rows_per_s": round(rows / med, 1), "spread": round((max(ts) - min(ts)) / med, 4)}
finite = bool(torch.isfinite(occlusion()).all().item())
plain_s = min(res["plain_forward"]["s"], res["plain_forward_again"]["s"])
print(json.dumps({"workload": f"Occlusion, wav2vec2-base shape, f32, {B} clips x 4 s, window {WIN}, stride {STRIDE}, "
                              f"K = {K}, {rows} ablated rows, internal batch {CHUNK} ({nchunk} chunks)",
                  "ablated_rows_per_s": res["occlusion"]["rows_per_s"], "ratio_to_plain_forward": round(plain_s / res["occlusion"]["s"], 4),
                  "runs": res, "finite": finite}))
