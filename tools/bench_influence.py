#!/usr/bin/env python3
"""The influence methods next to the plain forward over the same clips, in one process: wav2vec2-base shape, fp32-class, 4 s clips.
  (a) indexing: ``HipInfluenceIndex.add`` of ``--clips`` clips with pooled features alone, and of ``--layer-clips`` clips with
      ``layers=(6,)`` flattened (152 832 floats per clip), each next to ``EmbedderGrad.forward`` over the same chunks of 16 (A-B-A);
  (b) queries of 16 clips against a cached index of N = 65 536 synthetic pooled rows (and as many time-mean rows of the last layer):
      TracInCPFast with 3 checkpoints, influence functions and cosine similarity, each with k = 10; and against 1 024 synthetic
      flattened layer-6 rows: cosine and euclidean.  The post-forward launches are timed one by one next to the forward of the 16
      clips; for the influence functions also the moment kernel over the index, the host's factorisation (once per theta) and its solve per query (wall clock).
Times come from device events around each call; each figure is the median of ``--reps`` timed runs after two warm-up calls."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from addvisor_hip import concept as CO, influence as INF, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=1024)
ap.add_argument("--layer-clips", type=int, default=128)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=65536)
args = ap.parse_args()

torch.set_grad_enabled(False)
L, LAYER, CHUNK, B, K, REPS = 64000, 6, 16, 16, 10, args.reps
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
H, NL = cfg.hidden_size, att.eg.emb.nl
w = syn.make_clips(B, L, seed=12).to(dev)
yw = (torch.arange(B) % 2).float()


def timed(fn, reps=REPS):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) / 1e3)
    return {"s": round(statistics.median(ts), 6), "spread": round((max(ts) - min(ts)) / statistics.median(ts), 4)}


res = {}
# ---- (a) indexing ------------------------------------------------------------------------------------------------------------
for tag, n, layers in (("pooled", args.clips, ()), ("layer6", args.layer_clips, (LAYER,))):
    clips = syn.make_clips(n, L, seed=101).to(dev)
    labels = (torch.arange(n) % 2).float()

    def forward():
        for r0 in range(0, n, CHUNK):
            att.eg.forward(clips[r0:r0 + CHUNK])

    def add():
        return INF.HipInfluenceIndex(att, layers, internal_batch_size=CHUNK, memory_budget=32 << 30).add(clips, labels)

    a, b, c = timed(forward, 3), timed(add, 3), timed(forward, 3)
    res[f"index_{tag}"] = {"clips": n, "forward": a, "add": b, "forward_again": c, "ratio_to_forward": round(min(a["s"], c["s"]) / b["s"], 4),
                           "clips_per_s": round(n / b["s"], 1)}
    del clips

# ---- (b) queries against synthetic rows ------------------------------------------------------------------------------------------
N = args.rows
g = torch.Generator().manual_seed(5)
tmp = tempfile.mkdtemp()


def synthetic_index(layers, pool, rows, feats, frames):
    """An index whose rows are random numbers of the real rows' scale, through the public ``load``."""
    ix = INF.HipInfluenceIndex(att, layers, pool=pool, memory_budget=32 << 30)
    phi = np.concatenate([0.3 * torch.randn(rows, H, generator=g).numpy(), np.ones((rows, 1), np.float32)], 1)
    arrays = {"phi": phi, "labels": (np.arange(rows) % 2).astype(np.float32), "settings": np.str_(ix._settings(rows, frames))}
    for l in layers:
        arrays[f"layer_{l}"] = torch.randn(rows, feats, generator=g).numpy()
    path = os.path.join(tmp, f"{pool}_{rows}.npz")
    np.savez(path, **arrays)
    ix.load(path)
    os.remove(path)
    return ix


big = synthetic_index([NL], "mean", N, H, None)
res["forward_16"] = timed(lambda: att.eg.forward(w))
cps = [(0.05 * torch.randn(H, generator=g), 0.1 * c, 0.5 / (c + 1)) for c in range(3)]
tr = INF.HipTracInCPFast(big, cps)
li = INF.HipLogisticInfluence(big, 0.1)
cos = INF.HipSimilarityInfluence(big, NL, "cosine")
for name, fn in (("tracin_k10", lambda: tr.influence(w, yw, k=K)), ("influence_functions_k10", lambda: li.influence(w, yw, k=K)),
                 ("cosine_pooled_k10", lambda: cos.influence(w, top_k=K))):
    res[name] = timed(fn)
# the launches after the forward, one by one
Pt, At, _ = big.embed(w)
Pn, Yn, Xt = big.phi, big.activations(NL), At[NL]
yd = yw.to(dev)
Gx = CO.gram(Pt, Pn)
Zt, Zn = CO.gram(Pt, tr.W), CO.gram(Pn, tr.W)
rt, rn = INF.residual(Zt, yd), INF.residual(Zn, big.labels)
S = INF.scale(Gx, rt, rn, tr.lr)
one = torch.ones(1, dtype=torch.float64, device=dev)
ssn = INF.sumsq(Yn)
wts = torch.rand(N, generator=g).to(dev)
kern = {"gram_16xN_pooled": lambda: CO.gram(Pt, Pn), "gram_logits_16x3": lambda: CO.gram(Pt, tr.W), "gram_logits_Nx3_cached": lambda: CO.gram(Pn, tr.W),
        "residual_16x3": lambda: INF.residual(Zt, yd), "residual_Nx3_cached": lambda: INF.residual(Zn, big.labels),
        "scale_16xN_C3": lambda: INF.scale(Gx, rt, rn, tr.lr), "scale_16xN_C1": lambda: INF.scale(Gx, rt[:1], rn[:1], one),
        "topk_16xN_k10": lambda: INF.topk(S, K), "sumsq_16": lambda: INF.sumsq(Xt), "sumsq_N_cached": lambda: INF.sumsq(Yn),
        "cosine_16xN": lambda: INF.cosine(Gx, INF.sumsq(Xt), ssn), "moment_Nx769": lambda: INF.moment(Pn, wts)}
for name, fn in kern.items():
    res[name] = timed(fn)
host = []
Hm = li.hessian()
rhs = Pt.cpu().numpy().astype(np.float64).T
for _ in range(REPS):
    t0 = time.perf_counter()
    Li = np.linalg.solve(np.linalg.cholesky(Hm), np.eye(len(Hm)))            # once per theta
    t1 = time.perf_counter()
    Li.T @ (Li @ rhs)                                                        # per query
    host.append((t1 - t0, time.perf_counter() - t1))
res["host_factor_769_once_per_theta"] = {"s": round(statistics.median(h[0] for h in host), 6)}
res["host_solve_769_per_query"] = {"s": round(statistics.median(h[1] for h in host), 6)}
del big, tr, li, cos, Gx, S, Zn, rn, Pn, Yn

T = att.eg.forward(w, to_layer=LAYER).shape[1]
flat = synthetic_index([LAYER], "none", 1024, T * H, T)
for metric in ("cosine", "euclidean"):
    eng = INF.HipSimilarityInfluence(flat, LAYER, metric, "max" if metric == "cosine" else "min")
    res[f"{metric}_layer6_1024_k10"] = timed(lambda: eng.influence(w, top_k=K))
Yf, Xf = flat.activations(LAYER), flat.embed(w)[1][LAYER]
for name, fn in (("gram_16x1024_flat", lambda: CO.gram(Xf, Yf)), ("sqdist_16x1024_flat", lambda: INF.sqdist(Xf, Yf)),
                 ("sumsq_16_flat", lambda: INF.sumsq(Xf)), ("sumsq_1024_flat_cached", lambda: INF.sumsq(Yf))):
    res[name] = timed(fn)
fwd = res["forward_16"]["s"]
post = {"tracin": ["gram_16xN_pooled", "gram_logits_16x3", "residual_16x3", "scale_16xN_C3", "topk_16xN_k10"],
        "influence_functions": ["gram_16xN_pooled", "gram_logits_16x3", "residual_16x3", "scale_16xN_C1", "topk_16xN_k10"],
        "cosine_pooled": ["gram_16xN_pooled", "sumsq_16", "cosine_16xN", "topk_16xN_k10"],
        "cosine_layer6": ["gram_16x1024_flat", "sumsq_16_flat"], "euclidean_layer6": ["sqdist_16x1024_flat"]}
print(json.dumps({"workload": f"influence, wav2vec2-base shape, f32, 4 s clips; index of {N} synthetic pooled rows and 1024 flattened layer-{LAYER} rows "
                              f"({T * H} floats); queries of {B} clips, k = {K}",
                  "post_forward_share_of_forward": {k: round(sum(res[n]["s"] for n in v) / fwd, 4) for k, v in post.items()},
                  "runs": res}))
