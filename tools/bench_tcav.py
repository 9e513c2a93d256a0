#!/usr/bin/env python3
"""TCAV next to the plain passes over the same rows, in one process: wav2vec2-base shape, fp32-class, 4 s clips, layer 6,
``pool="none"`` (features = 199 x 768 = 152 832 per clip).
  (a) ``compute_cavs`` for 2 concepts x 64 clips (activations in chunks of 16 clips, the 128 x 128 Gram matrix, the host solve,
      the combine launch) next to ``forward(to_layer=6)`` over the same 128 clips in the same chunks;
  (b) ``interpret`` for 16 clips x 4 experimental sets (CAVs trained beforehand: one layer gradient, one Gram launch of the
      16 gradients against the 8 CAVs, the score statistics) next to ``layer_gradient_x_activation(w, 6, multiply_by_inputs=False)``
      over the same clips;
  the host solve of (a) on its own (wall clock, no device work);
  (c) the Gram launch (128 rows, symmetric), the combine launch (2 x 128 coefficients) and the score launch (16 x 8) on their own,
      with the bytes each must move computed from the shapes and that traffic's time at the measured HBM copy rate (6.29 TB/s) as a
      share of the launch.
Times come from device events around each call; each figure is the median of 7 timed runs after two warm-up calls, the plain pass
before and after (A-B-A)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import concept as CO, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

torch.set_grad_enabled(False)
L, LAYER, N, CHUNK, B, SETS, REPS, HBM = 64000, 6, 64, 16, 16, 4, 7, 6.29e12
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
concepts = [CO.Concept(i, f"c{i}", syn.make_clips(N, L, seed=100 + i).to(dev)) for i in range(SETS + 1)]
sets = [[concepts[0], concepts[k]] for k in range(1, SETS + 1)]                # one concept against four random counterparts
w = syn.make_clips(B, L, seed=12).to(dev)


def plain_forward():
    for c in concepts[:2]:
        for r0 in range(0, N, CHUNK):
            att.eg.forward(c.data_iter[r0:r0 + CHUNK], to_layer=LAYER)


def compute_cavs():
    return CO.HipTCAV(att, [LAYER], internal_batch_size=CHUNK).compute_cavs(sets[:1])      # a fresh engine: nothing cached


trained = CO.HipTCAV(att, [LAYER], internal_batch_size=CHUNK)
trained.compute_cavs(sets)


def interpret():
    return trained.interpret(w, sets)


def plain_gradient():
    return att.layer_gradient_x_activation(w, LAYER, multiply_by_inputs=False)


X = torch.cat([trained._concept_activations(c)[LAYER] for c in concepts[:2]])      # [128, F]
F = X.shape[1]
A = torch.randn(2, 2 * N, device=dev) / (2 * N)
G = plain_gradient().view(B, F)
W = torch.cat([trained.cavs[CO.concepts_to_str(s)][LAYER].weights for s in sets])   # [8, F]


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
for name, fn in (("forward_to_layer_128", plain_forward), ("compute_cavs_2x64", compute_cavs), ("forward_to_layer_128_again", plain_forward),
                 ("layer_gradient_16", plain_gradient), ("interpret_16x4", interpret), ("layer_gradient_16_again", plain_gradient),
                 ("gram_128", lambda: CO.gram(X)), ("combine_2x128", lambda: CO.combine(A, X)), ("gram_scores_16x8", lambda: CO.gram(G, W))):
    med, ts = timed(fn)
    res[name] = {"s": round(med, 6), "spread": round((max(ts) - min(ts)) / med, 4)}
fwd = min(res["forward_to_layer_128"]["s"], res["forward_to_layer_128_again"]["s"])
grad = min(res["layer_gradient_16"]["s"], res["layer_gradient_16_again"]["s"])
n = 2 * N
bytes_ = {"gram_128": n * F * 4 + 2 * CO.gram_workspace(n, n, F) + n * n * 8,              # rows once, partials written and read, G
          "combine_2x128": n * F * 4 + 2 * F * 4 + 2 * n * 4,
          "gram_scores_16x8": (B + 2 * SETS) * F * 4 + 2 * CO.gram_workspace(B, 2 * SETS, F) + B * 2 * SETS * 8}
# the host solve of (a) on its own: the 128 x 128 Gram matrix, the split, the dual Newton iterations (no device work)
K = CO.gram(X).cpu().numpy()
labels = (torch.arange(n) // N).numpy()
host = []
for _ in range(REPS):
    t0 = time.perf_counter()
    CO.fit_duals(CO.LogisticCAV(0.01), K, labels, 2, *CO.split_rows(n, 0.33, 0))
    host.append(time.perf_counter() - t0)
out = trained.interpret(w, sets)
finite = all(bool(torch.isfinite(v[LAYER]["scores"]).all().item()) for v in out.values())
print(json.dumps({"workload": f"TCAV, wav2vec2-base shape, f32, 4 s clips, layer {LAYER}, pool none, F = {F}; (a) compute_cavs, 2 concepts x {N} "
                              f"clips in chunks of {CHUNK}; (b) interpret, {B} clips x {SETS} experimental sets",
                  "a_ratio_to_forward": round(fwd / res["compute_cavs_2x64"]["s"], 4),
                  "a_clips_per_s": round(2 * N / res["compute_cavs_2x64"]["s"], 1),
                  "a_host_solve_s": round(statistics.median(host), 6),
                  "b_ratio_to_layer_gradient": round(grad / res["interpret_16x4"]["s"], 4),
                  "c_bytes": bytes_,
                  "c_hbm_share": {k: round(v / HBM / res[k]["s"], 4) for k, v in bytes_.items()},
                  "runs": res, "finite": finite}))
