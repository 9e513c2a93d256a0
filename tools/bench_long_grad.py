"""The gradient chain above 256 frames: what the streamed attention backward (csrc/attention_bwd_long.hip) costs.

    python tools/bench_long_grad.py [--precision f32,f16] [--rounds 15] [--warmup 3] [--launches 40] [--parts a,b]

One MI355X.  Every figure is the median over alternating rounds of a host clock around work that ends in a device synchronise,
printed with its min and max (the spread to hold a difference against).  Operands are random, not zeros.

  (a) kernel pair    the two launches of advh_attention_bwd_long_split at B = 16, T = 499 (10 s), 12 heads of 64, next to
                     advh_attention_bwd_split at T = 256 in the same build, once with advh_set_option("attention_bwd_mfma_f32", 1)
                     (the same arithmetic: every product on the fp32-input MFMA) and once at the default (three fp16 MFMAs per
                     product); all as (query, key) pairs per second.  The streamed form makes nine products per pair, the
                     whole-clip one seven: the aim for long / whole-f32 is 7 / 9 less the whole-f32 run's own (max - min) / median.
                     Also 16 heads of 120 (D = 128; the whole-clip entry runs the fp32-MFMA kernel there) and the fp16 entry
                     (next to advh_attention_bwd_f16 at T = 256, fp16 MFMAs).
  (b) chain          EmbedderGrad(long_clips=True): forward + backward of 16 clips x 10 s, next to the padded forward + backward
                     of 40 clips x 4 s on the existing path (7 984 against 7 960 frames), wav2vec2-base shape, per precision; and
                     the attention backward's share of the long call: layers x the launch pair's time of (a) / the call's time.
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_long_clips import alternate, stat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32,f16")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xai-audio-deepfakes_amd"))
    import torch
    from addvisor_hip import _lib, gemm as G, synthetic as syn
    from addvisor_hip.embedder import HipEmbedder
    from addvisor_hip.embedder_grad import EmbedderGrad
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_grad needs a GPU: a time from anything else says nothing")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    parts = set(args.parts.split(","))
    _lib.init()
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    B, T_long, T_whole = 16, 499, 256
    out = {"rounds": args.rounds, "launches": args.launches}
    pair_us = {}                                             # precision -> us per launch pair at 12 x 64 (the base model's layer)

    def operands(T, H, sp, g):
        mk = lambda rows: (G.split_planes(rows.double()) if sp else rows.half()).to(dev)
        qkv, dctx = mk(torch.randn(B * T, 3 * H, generator=g) * 0.7), mk(torch.randn(B * T, H, generator=g))
        return qkv, dctx, torch.empty(((2,) if sp else ()) + (B * T, 3 * H), dtype=torch.float16, device=dev)

    def kernel_part(name, sp, heads, dm, whole_variants):
        """Alternating rounds of ``launches`` long launch pairs at T = 499 and of each whole-clip variant at T = 256."""
        H = heads * dm
        g = torch.Generator().manual_seed(args.seed)
        (ql, dl, ol), (qw, dw, ow) = operands(T_long, H, sp, g), operands(T_whole, H, sp, g)
        ws = torch.empty(lib.advh_attention_bwd_long_ws_bytes(B, T_long, heads) // 4, dtype=torch.float32, device=dev)

        def long_():
            for _ in range(args.launches):
                rc = (lib.advh_attention_bwd_long_split(ql.data_ptr(), ql.stride(0), dl.data_ptr(), dl.stride(0), ol.data_ptr(), ol.stride(0),
                                                        ws.data_ptr(), None, B, T_long, H, heads, st) if sp else
                      lib.advh_attention_bwd_long_f16(ql.data_ptr(), dl.data_ptr(), ol.data_ptr(), ws.data_ptr(), None, B, T_long, H, heads, st))
            assert rc == 0

        def whole(force_f32):
            def run():
                if sp:
                    lib.advh_set_option(b"attention_bwd_mfma_f32", int(force_f32))
                for _ in range(args.launches):
                    rc = (lib.advh_attention_bwd_split(qw.data_ptr(), qw.stride(0), dw.data_ptr(), dw.stride(0), ow.data_ptr(), ow.stride(0),
                                                       B, T_whole, H, heads, st) if sp else
                          lib.advh_attention_bwd_f16(qw.data_ptr(), dw.data_ptr(), ow.data_ptr(), B, T_whole, H, heads, st))
                if sp:
                    lib.advh_set_option(b"attention_bwd_mfma_f32", 0)
                assert rc == 0
            return run
        runs = {"long": long_}
        runs.update({k: whole(f) for k, f in whole_variants.items()})
        t = alternate(runs, args.rounds, args.warmup, sync)
        _lib.check_overflow("bench_long_grad (a)")
        pairs = {k: B * heads * (T_long if k == "long" else T_whole) ** 2 for k in runs}
        a = {k: {"us_per_launch": stat([x * 1e3 / args.launches for x in v]),
                 "gpairs_per_s": round(pairs[k] * args.launches / (statistics.median(v) * 1e-3) / 1e9, 2)} for k, v in t.items()}
        for k in whole_variants:
            a["ratio_long_over_" + k] = round(a["long"]["gpairs_per_s"] / a[k]["gpairs_per_s"], 4)
        if "whole_f32" in a:
            w = a["whole_f32"]["us_per_launch"]
            a["aim_long_over_whole_f32"] = round(7.0 / 9.0 - (w["max"] - w["min"]) / w["median"], 4)
        print(name, "(a)", json.dumps(a), flush=True)
        return a

    if "a" in parts or "b" in parts:
        ka = out["kernel"] = {}
        ka["split_12x64"] = kernel_part("split 12 x 64", True, 12, 64, {"whole_f32": True, "whole_x3": False})
        ka["f16_12x64"] = kernel_part("f16 12 x 64", False, 12, 64, {"whole_f16": False})
        pair_us = {"f32": ka["split_12x64"]["long"]["us_per_launch"]["median"], "f16": ka["f16_12x64"]["long"]["us_per_launch"]["median"]}
        if "a" in parts:
            ka["split_16x120"] = kernel_part("split 16 x 120", True, 16, 120, {"whole_f32": False})      # head dims > 64: the fp32-MFMA kernel
            ka["f16_16x120"] = kernel_part("f16 16 x 120", False, 16, 120, {})                           # the whole-clip f16 entry refuses T > 208 there

    if "b" in parts:
        cfg = syn.base_config()
        nl = min(cfg.layer_index, cfg.num_hidden_layers)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        sd = syn.embedder_weights(cfg)
        cb = out["chain"] = {}
        for precision in args.precision.split(","):
            eg = EmbedderGrad(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision), long_clips=True)
            w_long, w_short = syn.make_clips(16, 160000).to(dev), syn.make_clips(40, 64000).to(dev)

            def call(w):
                def run():
                    eg.forward(w)
                    eg.backward()
                return run
            t = alternate({"long": call(w_long), "short": call(w_short)}, args.rounds, args.warmup, sync)
            b = {k + "_ms": stat(v) for k, v in t.items()}
            b["frames"] = [16 * eg._workspace(16, 160000)["f"]["T"], 40 * eg._workspace(40, 64000)["f"]["T"]]
            b["long_over_short"] = round(b["long_ms"]["median"] / b["short_ms"]["median"], 4)
            b["attention_bwd_ms"] = round(nl * pair_us[precision] * 1e-3, 4)
            b["attention_bwd_share_of_long"] = round(b["attention_bwd_ms"] / b["long_ms"]["median"], 4)
            cb[precision] = b
            print(precision, "(b)", json.dumps(b), flush=True)
            del eg, w_long, w_short
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
