"""Ragged batches in the gradient chain: what per-clip lengths cost against the padded ``forward + backward``, and what they save
against one call per clip.

    python tools/bench_ragged_grad.py [--model base] [--precision f32 f16] [--clips 64] [--length 64000] [--rounds 10]
                                      [--warmup 2] [--padded-only] [--tree DIR]

Workload (that of tools/bench_ragged.py): ``--clips`` clips in a batch of ``--length`` samples, the same seeded lengths (eight
values between a quarter of the batch length and the batch length), wav2vec2-base shape, for each precision.  Three things are
timed; the first two alternate round by round so that clock and host drift hit both alike, the third has a window of its own:

  padded      ``EmbedderGrad.forward(wave)`` + ``backward()``: every clip padded to the batch length;
  ragged      ``forward(wave, lengths=...)`` + ``backward()``: the same launches over the same (B, L) with the ragged siblings;
  per_clip    one warmed-up batch-1 ``forward + backward`` per clip at its true length (the only correct way before): one
              workspace and one plan set per distinct length, built before the timed window.

Each figure is the median over the rounds of a host clock around work that ends in a device synchronise; min and max are
printed with it (the spread to hold a difference against).  One JSON line per precision.  ``--padded-only`` times the first
alone; with ``--tree DIR`` the package is imported from another checkout (built there), which is how the padded path of two
commits is compared in one session.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("base", "tiny", "tiny_layer"), default="base")
    ap.add_argument("--precision", nargs="+", choices=("f32", "f16"), default=["f32", "f16"])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--padded-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "xai-audio-deepfakes_amd"))
    import numpy as np
    import torch
    from addvisor_hip import synthetic as syn
    from addvisor_hip.embedder import HipEmbedder
    from addvisor_hip.embedder_grad import EmbedderGrad
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_grad needs a GPU: a time from anything else says nothing")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = {"base": syn.base_config, "tiny": lambda: syn.tiny_config(False), "tiny_layer": lambda: syn.tiny_config(True)}[args.model]()
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    sd = syn.embedder_weights(cfg)
    B, L = args.clips, args.length
    values = [int(v) for v in np.linspace(L // 4, L, 8)]
    lengths = np.random.Generator(np.random.PCG64(args.seed)).choice(values, size=B).tolist()
    wave = syn.make_clips(B, L).to(dev)
    singles = [wave[b:b + 1, :n].contiguous() for b, n in enumerate(lengths)]
    for precision in args.precision:
        eg = EmbedderGrad(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))

        def padded():
            eg.forward(wave)
            eg.backward()

        def ragged():
            eg.forward(wave, lengths=lengths)
            eg.backward()

        def per_clip():
            for w in singles:
                eg.forward(w)
                eg.backward()

        windows = [{"padded": padded}] if args.padded_only else [{"padded": padded, "ragged": ragged}, {"per_clip": per_clip}]
        times = {}
        for runs in windows:
            for fn in runs.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times.update({k: [] for k in runs})
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out = {"model": args.model, "precision": precision, "clips": B, "length": L, "rounds": args.rounds,
               "mean_length": sum(lengths) / B, "distinct_lengths": len(set(lengths)), "tree": os.path.basename(os.path.abspath(args.tree))}
        for k, v in times.items():
            out[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            print(f"[{precision}] {k:9s} median {statistics.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}", flush=True)
        if not args.padded_only:
            out["ragged_over_padded"] = round(out["ragged_ms"]["median"] / out["padded_ms"]["median"], 4)
            out["per_clip_over_ragged"] = round(out["per_clip_ms"]["median"] / out["ragged_ms"]["median"], 4)
        print(json.dumps(out), flush=True)
        del eg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
