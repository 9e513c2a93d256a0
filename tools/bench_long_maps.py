"""Attention maps, rollout and LRP above 256 frames: what the streamed kernels of csrc/attention_maps_long.hip cost.

    python tools/bench_long_maps.py [--precision f32,f16] [--rounds 15] [--warmup 3] [--launches 40] [--parts a,b,c,d]

One MI355X, wav2vec2-base shape (12 heads of 64), 16 clips x 10 s (T = 499).  Every figure is the median over alternating rounds
of a host clock around work that ends in a device synchronise, printed with its min and max (the spread to hold a difference
against), as tools/bench_long_grad.py does.  Operands are random, not zeros.  One JSON line at the end; exit status 1 when a gate
fails.

  (a) value backward  advh_attention_bwd_value_long next to advh_attention_bwd_long_split / _f16 on the same operands.  GATED: it
                      does a strict subset of that kernel pair's work, so its median must not exceed the pair's by more than the
                      pair's own max - min.
  (b) maps            advh_attention_maps_long (mean over heads of the gradient form; and the per-head probabilities) at T = 499
                      next to the whole-clip advh_attention_maps at 16 x 256 frames, as (query, key, head) triples per second;
                      aim: ratio >= 1.0 (the whole-clip fused launch fills 64 of 256 CUs).
  (c) rollout step    advh_rollout_step_long at B = 16, T = 499 (2 T^3 flop per clip), next to advh_rollout_step at T = 256.
  (d) methods         HipAttribution(long_clips=True, long_maps=True): transformer_lrp and attention_grad_rollout on 16 x 10 s
                      next to layer_gradient_x_activation(w, 0) on the same chain.  GATED: each under twice that call.  Reported:
                      transformer_lrp over it (aim <= 1.0).
The statistics kernel has no entry of its own, so a host clock cannot time it apart; its share of a launch pair comes from a kernel
trace of parts (a) and (b) (`rocprofv3 --kernel-trace --stats -- python tools/bench_long_maps.py --parts a,b`): 73 us of the value
pair's 246 us (30 %), of the fused gradient maps pair's 288 us (25 %) and of the per-head probabilities pair's 221 us (33 %), DESIGN 4.35.
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
    ap.add_argument("--parts", default="a,b,c,d")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xai-audio-deepfakes_amd"))
    import torch
    from addvisor_hip import _lib, gemm as G, synthetic as syn
    from addvisor_hip.attribution import HipAttribution
    from addvisor_hip.embedder import HipEmbedder
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_maps needs a GPU: a time from anything else says nothing")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    parts = set(args.parts.split(","))
    _lib.init()
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    B, T_long, T_whole, heads, dm = 16, 499, 256, 12, 64
    H = heads * dm
    out = {"rounds": args.rounds, "launches": args.launches, "gates": {}}
    med = lambda v: statistics.median(v)

    def operands(T, sp, g):
        mk = lambda rows: (G.split_planes(rows.double()) if sp else rows.half()).to(dev)
        qkv, dctx = mk(torch.randn(B * T, 3 * H, generator=g) * 0.7), mk(torch.randn(B * T, H, generator=g))
        return qkv, dctx, torch.empty(((2,) if sp else ()) + (B * T, 3 * H), dtype=torch.float16, device=dev)

    lo = lambda t, sp: t.stride(0) if sp else 0

    for name, sp in (("split", True), ("f16", False)):
        g = torch.Generator().manual_seed(args.seed)
        (ql, dl, ol), (qw, dw, _) = operands(T_long, sp, g), operands(T_whole, sp, g)
        ws = torch.empty(lib.advh_attention_bwd_long_ws_bytes(B, T_long, heads) // 4, dtype=torch.float32, device=dev)
        if "a" in parts:
            def value_long():
                for _ in range(args.launches):
                    rc = lib.advh_attention_bwd_value_long(ql.data_ptr(), lo(ql, sp), dl.data_ptr(), lo(dl, sp), ol.data_ptr(), lo(ol, sp),
                                                           ws.data_ptr(), None, B, T_long, H, heads, st)
                assert rc == 0

            def bwd_long():
                for _ in range(args.launches):
                    rc = (lib.advh_attention_bwd_long_split(ql.data_ptr(), ql.stride(0), dl.data_ptr(), dl.stride(0), ol.data_ptr(),
                                                            ol.stride(0), ws.data_ptr(), None, B, T_long, H, heads, st) if sp else
                          lib.advh_attention_bwd_long_f16(ql.data_ptr(), dl.data_ptr(), ol.data_ptr(), ws.data_ptr(), None, B, T_long, H, heads, st))
                assert rc == 0
            t = alternate({"value_long": value_long, "bwd_long": bwd_long}, args.rounds, args.warmup, sync)
            _lib.check_overflow("bench_long_maps (a)")
            a = {k: stat([x * 1e3 / args.launches for x in v]) for k, v in t.items()}
            a["value_over_bwd"] = round(a["value_long"]["median"] / a["bwd_long"]["median"], 4)
            ok = a["value_long"]["median"] <= a["bwd_long"]["median"] + (a["bwd_long"]["max"] - a["bwd_long"]["min"])
            out["gates"][f"value_long_not_slower_{name}"] = bool(ok)
            out.setdefault("value", {})[name] = a
            print(name, "(a) us per launch", json.dumps(a), flush=True)
        if "b" in parts:
            b = {}
            for form, fuse, grad in (("grad_mean", 1, True), ("probs_per_head", 0, False)):
                shape = lambda T: (B, T, T) if fuse else (B, heads, T, T)
                out_l = torch.empty(shape(T_long), dtype=torch.float32, device=dev)
                out_w = torch.empty(shape(T_whole), dtype=torch.float32, device=dev)

                def long_():
                    for _ in range(args.launches):
                        rc = lib.advh_attention_maps_long(ql.data_ptr(), lo(ql, sp), dl.data_ptr() if grad else None, lo(dl, sp) if grad else 0,
                                                          1.0 / 4096.0, fuse, out_l.data_ptr(), ws.data_ptr(), None, B, T_long, H, heads, st)
                    assert rc == 0

                def whole():
                    for _ in range(args.launches):
                        rc = lib.advh_attention_maps(qw.data_ptr(), lo(qw, sp), dw.data_ptr() if grad else None, lo(dw, sp) if grad else 0,
                                                     1.0 / 4096.0, fuse, out_w.data_ptr(), B, T_whole, H, heads, st)
                    assert rc == 0
                t = alternate({"long": long_, "whole": whole}, args.rounds, args.warmup, sync)
                r = {k: {"us_per_launch": stat([x * 1e3 / args.launches for x in v]),
                         "gtriples_per_s": round(B * heads * (T_long if k == "long" else T_whole) ** 2 * args.launches / (med(v) * 1e-3) / 1e9, 2)}
                     for k, v in t.items()}
                r["rate_long_over_whole"] = round(r["long"]["gtriples_per_s"] / r["whole"]["gtriples_per_s"], 4)
                b[form] = r
                del out_l, out_w
            out.setdefault("maps", {})[name] = b
            print(name, "(b)", json.dumps(b), flush=True)
        del ql, dl, ol, qw, dw, ws
        torch.cuda.empty_cache()

    if "c" in parts:
        g = torch.Generator().manual_seed(args.seed)
        mk = lambda T: torch.softmax(torch.randn(B, T, T, generator=g), -1).to(dev)
        (Ml, Xl), (Mw, Xw) = (mk(T_long), mk(T_long)), (mk(T_whole), mk(T_whole))
        Yl, Yw = torch.empty_like(Xl), torch.empty_like(Xw)

        def step_long():
            for _ in range(args.launches):
                rc = lib.advh_rollout_step_long(Ml.data_ptr(), Xl.data_ptr(), Yl.data_ptr(), 1.0, 1.0, 1.0, 0, None, B, T_long, st)
            assert rc == 0

        def step_whole():
            for _ in range(args.launches):
                rc = lib.advh_rollout_step(Mw.data_ptr(), Xw.data_ptr(), Yw.data_ptr(), 1.0, 1.0, 1.0, 0, B, T_whole, st)
            assert rc == 0
        t = alternate({"long": step_long, "whole": step_whole}, args.rounds, args.warmup, sync)
        c = {k: {"us_per_launch": stat([x * 1e3 / args.launches for x in v]),
                 "tflops": round(2.0 * B * (T_long if k == "long" else T_whole) ** 3 * args.launches / (med(v) * 1e-3) / 1e12, 3)}
             for k, v in t.items()}
        out["rollout_step"] = c
        print("(c)", json.dumps(c), flush=True)
        del Ml, Xl, Mw, Xw, Yl, Yw

    if "d" in parts:
        cfg = syn.base_config()
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        sd = syn.embedder_weights(cfg)
        md = out["methods"] = {}
        for precision in args.precision.split(","):
            att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision), long_clips=True, long_maps=True)
            w = syn.make_clips(16, 160000).to(dev)
            t = alternate({"layer_gradient_x_activation": lambda: att.layer_gradient_x_activation(w, 0),
                           "transformer_lrp": lambda: att.transformer_lrp(w),
                           "attention_grad_rollout": lambda: att.attention_grad_rollout(w),
                           "attention_rollout": lambda: att.attention_rollout(w)}, args.rounds, args.warmup, sync)
            d = {k + "_ms": stat(v) for k, v in t.items()}
            base = d["layer_gradient_x_activation_ms"]["median"]
            for k in ("transformer_lrp", "attention_grad_rollout", "attention_rollout"):
                d[k + "_over_plain"] = round(d[k + "_ms"]["median"] / base, 4)
            for k in ("transformer_lrp", "attention_grad_rollout"):
                out["gates"][f"{k}_under_twice_plain_{precision}"] = bool(d[k + "_ms"]["median"] < 2.0 * base)
            md[precision] = d
            print(precision, "(d)", json.dumps(d), flush=True)
            del att, w
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if not all(out["gates"].values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
