#!/usr/bin/env python3
"""Per-layer device time of the inference U-Net (B = 64, 512 x 196) on one MI355X.

``bench_unet_layers.py [B] --ab``: additionally builds the network in its previous form (GEMM plans that enumerate the padded
output grid, e2.block.0 on the implicit GEMM) and with interior-only GEMM plans but e2.block.0 still on the GEMM, and times every
layer whose plan differs between the forms, alternating, three runs of ten launches each: the merge rule of DESIGN §4.19 compares
the new form's median with the old form's fastest run."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch
from addvisor_hip import gemm as G, synthetic as syn
from addvisor_hip.unet import HipUNet
torch.set_grad_enabled(False)
AB = "--ab" in sys.argv
args = [a for a in sys.argv[1:] if a != "--ab"]
B = int(args[0]) if args else 64
dev = torch.device("cuda:0")
net = HipUNet(syn.unet_weights(), dev, fuse_up=os.environ.get("UNET_FUSE_UP", "1") != "0", precision=os.environ.get("UNET_PRECISION", "f32"))
mag = torch.rand(B, 513, 199, device=dev)
net.forward(mag); torch.cuda.synchronize()
ws = net._workspace(B, 512, 196)
m = ws["maps"]
tot = 0.0
for plan, srcs, dst in ws["steps"]:
    a0 = m[srcs[0]].t; a1 = m[srcs[1]].t if len(srcs) > 1 else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        plan.run(a0, a1, out_h=m[dst].t)
    e1.record(); e1.synchronize()
    ms = e0.elapsed_time(e1) / 5
    tot += ms
    kind = getattr(plan, "kind", "gemm")
    if kind == "gemm":
        kind = G.TILE_NAMES[plan.tile] + ("*" if isinstance(plan, G.PlanGroup) else "")
    kind += "+head" if getattr(plan, "head", None) else ""
    print(f"{'+'.join(srcs):8s} -> {dst:4s} {kind:14s} {ms*1e3:8.1f} us  {plan.flops/ms/1e9:7.1f} TFLOP/s  ({plan.flops/1e9:6.1f} GF)")
print(f"total GEMM-shaped layers {tot:.3f} ms")
if AB:
    def build(padded):
        """The network with e2.block.0 on the implicit GEMM and the GEMM plans padded (the previous form) or interior-only."""
        n = HipUNet(syn.unet_weights(), dev, fuse_up=net.fuse_up, precision=net.precision)
        n.conv_choice.update(s21_tile=False, interior_only=not padded)
        n.forward(mag); torch.cuda.synchronize()
        return n, n._workspace(B, 512, 196)

    old, wo = build(True)
    mid, wm = build(False)

    def timed(w, step):
        plan, srcs, dst = step
        a0 = w["maps"][srcs[0]].t; a1 = w["maps"][srcs[1]].t if len(srcs) > 1 else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            plan.run(a0, a1, out_h=w["maps"][dst].t)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 100.0

    form = lambda p: f"GEMM M={p.desc.M}" if isinstance(p, G.GemmPlan) else type(p).__name__
    print("previous form (padded GEMM) | interior-only GEMM | dispatched form where it is neither: us per launch, three alternating runs each, sorted")
    saved = 0.0
    for so, sm, sn in zip(wo["steps"], wm["steps"], ws["steps"]):
        forms = [(wo, so)]
        for w, st in ((wm, sm), (ws, sn)):
            if all(form(st[0]) != form(f[1][0]) for f in forms):
                forms.append((w, st))
        if len(forms) == 1:
            continue
        t = [[] for _ in forms]
        for _ in range(3):
            for k, (w, st) in enumerate(forms):
                t[k].append(timed(w, st))
        for r in t:
            r.sort()
        saved += t[0][1] - t[-1][1]
        cells = " | ".join(f"{form(st[0]):>22} {r[0]:7.1f} {r[1]:7.1f} {r[2]:7.1f}" for (w, st), r in zip(forms, t))
        print(f"{'+'.join(sn[1]):8s} -> {sn[2]:4s} {cells} | medians {t[0][1] - t[-1][1]:6.1f}  last median < first min: {t[-1][1] < t[0][0]}")
    print(f"sum of median differences, previous form - dispatched form: {saved:.1f} us")
