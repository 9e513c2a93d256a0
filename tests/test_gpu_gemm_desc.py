"""Every kernel instance of ``advh_gemm_f16`` (csrc/gemm.hip) against the fp64 replay of its descriptor (tests/gemm_desc_ref.py).

The plans are built through the ``GemmPlan`` constructor, not the planners, the tile is forced, and the descriptor is launched
through the C entry point from ``launch`` below so that no field under test (``sc``, ``w_ld``, the plane distances) is
recomputed on the way.  The case table (``gemm_desc_ref.CASES``) holds, per instance, the smallest shapes at which the code paths
differ: three M tiles with a ragged last one on a (B, Hg, Wg) grid with a one-row, one-column halo window, two or three N tiles with
a ragged last one (``BN + 8`` wide, ``BN + 4`` narrow), Ktot = 192 from 17 real chunks, ``nz = 4`` with ``nz_lo = 2``, workgroup
counts that are no multiple of 8, and ``sc = 2`` over three N tiles.  tests/test_gemm_desc_ref_cpu.py proves on the CPU that the
table reaches every (instance, epilogue form) pair and that each case tells every single descriptor mistake apart.

Per case: the host-side audit of every range the contract reads or writes precedes the launch; every output buffer is
pre-filled and every element outside the contract's written mask must keep its bits; every written element meets
``gemm_desc_ref.bound`` (derived from the arithmetic, see its docstring); halo zeros are +0; the 512-thread tiles are
bit-identical to the 128x128 tile on the same descriptor.

Worst |err| / bound per instance over all its cases and outputs, measured on an MI355X (the fp16 instances sit at the fp16
half-ulp of the store, which is most of their bound; the split instances at about 1 % of theirs, which the accumulation term
Ktot * 2^-24 * S dominates -- tests/test_gemm_desc_ref_cpu.py shows that bound still sees a lost lo plane):
  f16_128x128        0.945  row_z_inner out_h (staged_rows_leaky)     x3_128x128        0.010  row_z_inner out_h (staged_rows_leaky)
  f16_128x128_plain  0.950  plain_resid_h out_h (lean_wide)           x3_128x128_plain  0.013  plain_z out_h (staged_none)
  f16_256x64         0.944  row_z_inner out_h (staged_rows_leaky)     x3_256x64         0.012  arow_outf out_f (generic_wide)
  f16_256x32         0.942  row_z out_h (rows_tight_leaky)            x3_256x32         0.011  arow_resid_h2 out_h2 (generic_wide)
  f16_256x128_w8     0.947  row_none out_h (rows_tight_none)
  f16_128x256_w8     0.948  plainflag_none out_h (rows_tight_none)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_desc_ref as R
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def launch(plan, case, tens, dev, tile):
    """One ``advh_gemm_f16`` call on device copies of the case's buffers; returns the output buffers on the host."""
    sp = plan.spec
    alias = sp.resid in ("alias_h", "alias_f")
    dt = {k: t.clone().to(dev) for k, t in tens.items() if k not in ("W", "bias") and not (alias and k == "resid")}
    if alias:
        dt["resid"] = dt["out_h" if sp.resid == "alias_h" else "out_f"]
    d = G.GemmDesc.from_buffer_copy(plan.desc)
    d.A0, d.A1 = dt["A0"].data_ptr(), (dt["A1"].data_ptr() if "A1" in dt else None)
    d.W, d.ktab = plan.w.data_ptr(), plan.ktab.data_ptr()
    d.bias = plan.bias.data_ptr() if plan.bias is not None else None
    for k in ("resid", "dact_src") + R.OUTS:
        setattr(d, k, dt[k].data_ptr() if k in dt else None)
    rc = _lib.lib().advh_gemm_f16(C.byref(d), tile, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    _lib.check_overflow(case.id)
    return {o: dt[o].cpu() for o in sp.outs}


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_instance_matches_the_fp64_replay(gpu_device, case):
    _lib.init()
    inst = case.inst
    plan = R.build_plan(case, device=gpu_device)
    bufs, tens, planes, numel = R.host_buffers(case, plan)
    d = R.case_desc(case, plan)
    rep = R.replay(d, bufs, planes, inst.BN)
    R.audit(rep, numel)                                          # a wrong case fails here, on the host
    if inst.plain is not None:
        assert R.affine_loader(inst, d) == inst.plain
    got = launch(plan, case, tens, gpu_device, inst.tile)
    worst = 0.0
    for o, (ref, mask) in rep.out.items():
        g, init, P = got[o], tens[o], planes[o]
        npl = 1 if o == "out_f" else g.numel() // P
        gb, ib = bits(g).reshape(npl, P), bits(init).reshape(npl, P)
        for pl in range(npl):
            assert np.array_equal(gb[pl][~mask], ib[pl][~mask]), f"{case.id} {o}: an element outside the contract's mask changed (plane {pl})"
            assert not gb[pl][rep.zero[o]].any(), f"{case.id} {o}: a halo zero is not +0"
        val = g.double().numpy().reshape(npl, P)
        val = val[0] + (val[1] * 2.0 ** -11 if npl == 2 else 0.0)
        assert np.isfinite(val[mask]).all()
        err, bnd = np.abs(val - ref)[mask], R.bound(d, rep, o)[mask]
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
        i = int(ratio.argmax())
        worst = max(worst, float(ratio[i]))
        print(f"GEMMDESC {case.id} {o} form={R.form(inst, d)} worst |err|/bound = {ratio[i]:.3f} (|err| {err[i]:.3e}, bound {bnd[i]:.3e})")
        assert (err <= bnd).all(), f"{case.id} {o}: |err| / bound = {ratio[i]:.3f}"
    if inst.tile in (G.TILE_256x128_W8, G.TILE_128x256_W8):
        base = launch(plan, case, tens, gpu_device, G.TILE_128x128)
        for o in plan.spec.outs:
            assert np.array_equal(bits(got[o]), bits(base[o])), f"{case.id} {o}: not bit-identical to the 128x128 tile"
