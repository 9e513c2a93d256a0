"""The contract of ``advh_gemm_desc`` (include/addvisor_hip.h) replayed in numpy fp64, the form the kernels of csrc/gemm.hip
pick for a descriptor, and the case table of tests/test_gpu_gemm_desc.py.

``replay`` is written from the header's comment block: row enumeration and window, per-chunk source selection, the batch
strides (two-level with ``nz_lo``), ``w_ld``, the wide row permutation, bias / activation / GELU' / residual, ``out_pre`` /
``out_h2``, the column split (``n_div`` / ``n_sub``) and the phase window.  Operands are read exactly as stored (fp16, or the plane
pair ``hi + lo * 2**-11``).  It returns, per output buffer, the fp64 value, the mask of the elements the contract writes and the
magnitude sum ``S`` the error bound is built from, plus the element ranges the contract lets a kernel read and write.

Buffers are flat arrays addressed in elements from the pointer the descriptor holds; a split buffer holds both planes and the
descriptor's ``a_lo`` / ``w_lo`` / ``o_lo`` say where the lo plane starts."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from addvisor_hip import gemm as G

ACT_NONE, ACT_GELU, ACT_LEAKY = 0, 1, 2
OUTS = ("out_h", "out_f", "out_h2", "out_pre")
_PTRS = ("A0", "A1", "W", "ktab", "bias", "resid", "out_h", "out_f", "out_h2", "out_pre", "dact_src")


def desc_fields(desc) -> SimpleNamespace:
    """The descriptor as plain Python values; a pointer field becomes ``bool(pointer)``."""
    d = SimpleNamespace()
    for name, _ in desc._fields_:
        v = getattr(desc, name)
        if name in _PTRS:
            v = bool(v)
        elif hasattr(v, "__len__"):
            v = [int(x) for x in v]
        setattr(d, name, v)
    return d


# ------------------------------------------------------------------------------------------------ instances and forms
@dataclass(frozen=True)
class Instance:
    name: str
    tile: int
    split: bool
    plain: Optional[bool]      # the loader this instance is: True affine-row, False gathered, None: desc.plain picks (split 256-row tiles)
    BM: int
    BN: int
    NI: int                    # 16-column MFMA tiles per wavefront
    stage: bool                # the wavefront tile fits the K loop's LDS (csrc/gemm.hip: `stage`)


def _stage(BM, BN, WM, WN, split):
    MI, NI = BM // WM // 16, BN // WN // 16
    if split:
        return NI == 4 and MI * 16 * 256 * WM * WN <= 2 * (BM + BN) * 64 * 2
    return NI == 4 and MI * 16 * 128 * WM * WN <= (BM + BN) * 64 * 2


def _inst(name, tile, split, plain, BM, BN, WM, WN):
    return Instance(name, tile, split, plain, BM, BN, BN // WN // 16, _stage(BM, BN, WM, WN, split))


INSTANCES: Dict[str, Instance] = {i.name: i for i in (
    _inst("f16_128x128", G.TILE_128x128, False, False, 128, 128, 2, 2),
    _inst("f16_128x128_plain", G.TILE_128x128, False, True, 128, 128, 2, 2),
    _inst("f16_256x64", G.TILE_256x64, False, False, 256, 64, 4, 1),
    _inst("f16_256x32", G.TILE_256x32, False, False, 256, 32, 4, 1),
    _inst("f16_256x128_w8", G.TILE_256x128_W8, False, False, 256, 128, 4, 2),
    _inst("f16_128x256_w8", G.TILE_128x256_W8, False, False, 128, 256, 2, 4),
    _inst("x3_128x128", G.TILE_128x128, True, False, 128, 128, 2, 2),
    _inst("x3_128x128_plain", G.TILE_128x128, True, True, 128, 128, 2, 2),
    _inst("x3_256x64", G.TILE_256x64, True, None, 256, 64, 4, 1),
    _inst("x3_256x32", G.TILE_256x32, True, None, 256, 32, 4, 1),
)}


def affine_loader(inst: Instance, d) -> bool:
    """Does this launch run the affine-row loader (``PLAIN`` template argument)?"""
    return bool(d.plain) and (inst.split or inst.tile == G.TILE_128x128)


def tight_mode(d) -> int:
    if not d.wide or d.out_pre or d.dact_src or d.out_h2:
        return -1
    if d.out_h and not d.out_f and not d.resid:
        return 0 if d.act == ACT_NONE else 1 if d.act == ACT_GELU else -1
    if d.out_f and not d.out_h and d.resid and d.resid_f32 and d.act == ACT_NONE:
        return 2
    return -1


def form(inst: Instance, d) -> str:
    """Name of the epilogue form the kernel instance runs for this descriptor (mirror of tight_mode / gemm_epilogue_plain /
    gemm_epilogue_rows in csrc/gemm.hip)."""
    staged = inst.NI == 4 and inst.stage
    if affine_loader(inst, d) and d.plain_out:
        mode = tight_mode(d)
        if mode >= 0:
            return ("staged_none", "staged_gelu", "staged_f32")[mode] if staged else "tight%d" % mode
        return "lean_wide" if d.wide else "lean_narrow"
    act = {ACT_NONE: "none", ACT_GELU: "gelu", ACT_LEAKY: "leaky"}[d.act]
    oneblk = d.n_div >= d.N and d.ph_r <= 0
    plain_h = d.out_h and not d.out_f and not d.out_pre and not d.dact_src
    if d.wide and oneblk and plain_h and not d.resid and not d.out_h2:
        return ("staged_rows_" if staged else "rows_tight_") + act
    if staged and d.wide and oneblk and plain_h and d.act == ACT_NONE and (d.out_h2 or (d.resid and not d.resid_f32)) \
            and not (d.resid and d.resid_f32):
        return "rows_staged_resid"
    return "generic_wide" if d.wide else "generic_narrow"


_ROW_STAGED = {"staged_rows_none", "staged_rows_gelu", "staged_rows_leaky", "rows_staged_resid", "generic_wide", "generic_narrow"}
_ROW_TIGHT = {"rows_tight_none", "rows_tight_gelu", "rows_tight_leaky", "generic_wide", "generic_narrow"}
_PLAIN_STAGED = {"staged_none", "staged_gelu", "staged_f32", "lean_wide", "lean_narrow"}
_PLAIN_TIGHT = {"tight0", "tight1", "tight2", "lean_wide", "lean_narrow"}
# every (instance, form) pair that exists in csrc/gemm.hip, written out: a kernel change that adds or removes a form must
# change this table (tests/test_gemm_desc_ref_cpu.py::test_case_table_reaches_every_form)
EXPECTED_FORMS: Dict[str, set] = {
    "f16_128x128": _ROW_STAGED,
    "f16_128x128_plain": _ROW_STAGED | _PLAIN_STAGED,
    "f16_256x64": _ROW_STAGED,
    "f16_256x32": _ROW_TIGHT,
    "f16_256x128_w8": _ROW_TIGHT,
    "f16_128x256_w8": _ROW_TIGHT,
    "x3_128x128": _ROW_STAGED,
    "x3_128x128_plain": _ROW_STAGED | _PLAIN_STAGED,
    "x3_256x64": _ROW_STAGED | _PLAIN_STAGED,
    "x3_256x32": _ROW_TIGHT | _PLAIN_TIGHT,
}


# ------------------------------------------------------------------------------------------------ the fp64 replay
def _gelu(x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))).numpy()


def _gelu_grad(x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)).numpy()


def _read_h(buf, idx, lo, split):
    """fp16-side read: the element as stored, or hi + lo * 2**-11 of the plane pair."""
    assert idx.size == 0 or idx.min() >= 0, "negative element index"
    v = buf[idx].astype(np.float64)
    if split:
        v = v + buf[idx + lo].astype(np.float64) * 2.0 ** -11
    return v


def _merge(starts, width):
    """Sorted disjoint [lo, hi) ranges covering ``[s, s + width)`` for every start."""
    s = np.unique(np.asarray(starts, dtype=np.int64).reshape(-1))
    if s.size == 0:
        return []
    e = np.maximum.accumulate(s + width)
    cut = np.nonzero(s[1:] > e[:-1])[0]
    lo = np.concatenate([s[:1], s[cut + 1]])
    hi = np.concatenate([e[cut], e[-1:]])
    return list(zip(lo.tolist(), hi.tolist()))


@dataclass
class Replay:
    out: Dict[str, Tuple[np.ndarray, np.ndarray]]        # name -> (fp64 value, written mask), one logical plane
    S: Dict[str, np.ndarray]                             # name -> sum |a||w| + |bias| + |resid| per element
    amp: Dict[str, np.ndarray]                           # name -> |derivative factor| applied after the sum (GELU' of dact_src), else 1
    zero: Dict[str, np.ndarray]                          # name -> elements written as halo zeros
    reads: Dict[str, list] = field(default_factory=dict)     # buffer -> [lo, hi) element ranges a kernel may read
    writes: Dict[str, list] = field(default_factory=dict)    # buffer -> [lo, hi) element ranges the contract writes


def replay(d, bufs: Dict[str, np.ndarray], planes: Dict[str, int], BN: int, *, check: bool = True, drop_wide: bool = False,
           ranges: bool = True) -> Replay:
    """``d``: ``desc_fields`` of the descriptor; ``bufs``: flat arrays behind A0, A1, W, ktab (int64, bit 31 = source), bias, resid,
    dact_src; ``planes``: elements of one logical plane of every output buffer present; ``BN``: the tile's column count (weight
    rows up to its multiple may be read).  ``check=False`` skips the validity assertions (mutated descriptors);
    ``drop_wide`` reads the weight rows as if ``wide`` were 0 (the mistake of forgetting the permutation)."""
    M, N, K = d.M, d.N, d.Ktot
    nch = K // 8
    split = bool(d.split)
    m = np.arange(M, dtype=np.int64)
    w_, t_ = m % d.Wg, m // d.Wg
    h_, b_ = t_ % d.Hg, t_ // d.Hg
    ok = (h_ >= d.h0) & (h_ < d.h1) & (w_ >= d.w0) & (w_ < d.w1)
    kt = np.asarray(bufs["ktab"], dtype=np.int64)[:nch]
    sel, off = (kt >> 31) & 1, kt & 0x7FFFFFFF
    if check:
        assert K % 64 == 0 and N % 4 == 0 and d.n_div % 4 == 0
        assert not d.ktab_identity or bool((kt == np.arange(nch)).all())
        assert not d.plain or (d.ktab_identity and not sel.any())
        if d.plain_out:
            assert d.plain and d.n_div >= N and d.ph_r <= 0 and d.n_sub <= 1 and ok.all()
        if d.wide:
            assert all(v % 8 == 0 for v in (N, d.n_div, d.o_c0, d.o_sB, d.o_sH, d.o_sW, d.o_sNhi, d.o_sZ, d.o_sNhh, d.o_sZ2))
    wld = d.w_ld if d.w_ld else K
    rowsW = -(-N // BN) * BN
    assert rowsW <= d.w_rows
    chan = G.packed_row_channel(rowsW) if (d.wide and not drop_wide) else np.arange(rowsW)
    rowof = np.empty(rowsW, dtype=np.int64)
    rowof[chan] = np.arange(rowsW)
    rowof = rowof[:N]
    n = np.arange(N, dtype=np.int64)
    q = n // d.n_div
    colo = (((q // d.n_sub) * d.o_sNhh + (q % d.n_sub) * d.o_sNhi) if d.n_sub > 1 else q * d.o_sNhi) + n % d.n_div
    names = [o for o in OUTS if getattr(d, o)]
    val = {o: np.zeros(planes[o]) for o in names}
    mask = {o: np.zeros(planes[o], dtype=bool) for o in names}
    zero = {o: np.zeros(planes[o], dtype=bool) for o in names}
    Sd = {o: np.zeros(planes[o]) for o in names}
    amp = {o: np.ones(planes[o]) for o in names}
    rd = {k: [] for k in ("A0", "A1", "W", "bias", "resid", "dact_src", "ktab")}
    rd["ktab"].append((np.zeros(1, dtype=np.int64), nch))
    mv = np.nonzero(ok)[0]
    kk = np.arange(K, dtype=np.int64)
    for z in range(max(d.nz, 1)):
        zh, zw = (z // d.nz_lo, z % d.nz_lo) if d.nz_lo > 1 else (z, 0)
        zoff = [d.a_sZ[s] * zh + d.a_sZ2[s] * zw for s in (0, 1)]
        rb = [b_ * d.a_sB[s] + h_ * d.a_sH[s] + w_ * d.a_sW[s] + d.a_c0[s] + zoff[s] for s in (0, 1)]
        if d.plain:                                     # every row m < M may be read at its affine address, K contiguous chunks
            aff = d.a_c0[0] + m * d.a_sW[0] + zoff[0]
            if check:
                assert (aff[ok] == rb[0][ok]).all(), "plain = 1 needs a_sB / a_sH consistent with a_sW"
            rd["A0"].append((aff * 8, K))
        chunk = np.where(sel[None, :] == 0, rb[0][mv][:, None], rb[1][mv][:, None]) + off[None, :]
        el = (chunk[:, :, None] * 8 + np.arange(8)).reshape(len(mv), K)
        A = np.zeros((len(mv), K))
        for s in (0, 1):
            cs = np.nonzero(sel == s)[0]
            if cs.size == 0:
                continue
            cols = (cs[:, None] * 8 + np.arange(8)).reshape(-1)
            A[:, cols] = _read_h(bufs["A%d" % s], el[:, cols], d.a_lo[s] * 8, split)
            safe = d.h0 * d.a_sH[s] + d.w0 * d.a_sW[s] + d.a_c0[s] + zoff[s]       # the row invalid rows and the M tail read
            rd["A%d" % s].append((np.concatenate([chunk[:, cs].reshape(-1), safe + off[cs]]) * 8, 8))
        wbase = d.w_sZ * z
        Wn = _read_h(bufs["W"], wbase + rowof[:, None] * wld + kk[None, :], d.w_lo, split)
        rd["W"].append((wbase + np.arange(rowsW, dtype=np.int64) * wld, K))
        acc = A @ Wn.T
        S = np.abs(A) @ np.abs(Wn).T
        if d.bias:
            bv = bufs["bias"][d.bias_sZ * z + n].astype(np.float64)
            acc = acc + bv
            S = S + np.abs(bv)
            rd["bias"].append((np.array([d.bias_sZ * z]), N))
        pre = acc
        v = _gelu(acc) if d.act == ACT_GELU else np.where(acc > 0, acc, float(d.slope) * acc) if d.act == ACT_LEAKY else acc
        zo = d.o_sZ * zh + d.o_sZ2 * zw
        orow = b_ * d.o_sB + h_ * d.o_sH + w_ * d.o_sW + d.o_c0 + zo
        if check and d.plain_out:
            assert (orow == d.o_c0 + m * d.o_sW + zo).all(), "plain_out = 1 needs o_sB / o_sH consistent with o_sW"
        O = orow[mv][:, None] + colo[None, :]
        keep = np.ones(O.shape, dtype=bool)
        if d.ph_r > 0:
            to = w_[mv][:, None] * d.ph_r + q[None, :] - d.ph_pad
            keep = (to >= 0) & (to < d.ph_T)
        Of, vf, pf, Sf = O[keep], v[keep], pre[keep], S[keep]
        Spre = Sf
        af = np.ones_like(vf)
        if d.dact_src:
            gf = _gelu_grad(_read_h(bufs["dact_src"], Of, d.o_lo, split))
            vf, af = vf * gf, np.abs(gf)
            rd["dact_src"].append((Of, 1))
        if d.resid:
            r = bufs["resid"][Of].astype(np.float64) if d.resid_f32 else _read_h(bufs["resid"], Of, d.o_lo, split)
            assert Of.size == 0 or Of.min() >= 0
            vf = vf + r
            Sf = Sf * af + np.abs(r)
            af = np.ones_like(vf)
            rd["resid"].append((Of, 1))
        for o in names:
            assert Of.size == 0 or Of.min() >= 0, "negative output offset"
            if check:
                assert not mask[o][Of].any() and np.unique(Of).size == Of.size, "two rows / batches write one element"
            mask[o][Of] = True
            if o == "out_pre":
                val[o][Of], Sd[o][Of] = pf, Spre
            elif o == "out_h2":
                val[o][Of], Sd[o][Of], amp[o][Of] = np.where(vf > 0, vf, float(d.slope2) * vf), Sf, af
            else:
                val[o][Of], Sd[o][Of], amp[o][Of] = vf, Sf, af
        if d.halo_zero and (~ok).any():
            hv = np.nonzero(~ok)[0]
            Oh = orow[hv][:, None] + colo[None, :]
            if d.ph_r > 0:
                to = w_[hv][:, None] * d.ph_r + q[None, :] - d.ph_pad
                Oh = Oh[(to >= 0) & (to < d.ph_T)]
            Oh = Oh.reshape(-1)
            for o in names:
                if o == "out_pre":
                    continue                             # no value before `act` exists for a halo row
                assert Oh.size == 0 or Oh.min() >= 0
                if check:
                    assert not mask[o][Oh].any()
                mask[o][Oh], zero[o][Oh], val[o][Oh] = True, True, 0.0
    res = Replay({o: (val[o], mask[o]) for o in names}, Sd, amp, zero)
    if ranges:
        lo_of = {"A0": d.a_lo[0] * 8, "A1": d.a_lo[1] * 8, "W": d.w_lo, "dact_src": d.o_lo, "resid": 0 if d.resid_f32 else d.o_lo}
        for k, lst in rd.items():
            r = []
            for starts, width in lst:
                r += _merge(starts, width)
                if split and lo_of.get(k):
                    r += _merge(np.asarray(starts) + lo_of[k], width)
            res.reads[k] = sorted(r)
        for o in names:
            idx = np.nonzero(mask[o])[0]
            r = _merge(idx, 1)
            if split and o != "out_f":
                r += _merge(idx + d.o_lo, 1)
            res.writes[o] = r
    return res


def audit(rep: Replay, numel: Dict[str, int]) -> None:
    """Every range the contract reads or writes lies inside its buffer; raises AssertionError naming the buffer."""
    for kind, table in (("read", rep.reads), ("write", rep.writes)):
        for name, rs in table.items():
            for lo, hi in rs:
                assert 0 <= lo and hi <= numel[name], f"{kind} of {name} [{lo}, {hi}) outside its {numel.get(name)} elements"


# ------------------------------------------------------------------------------------------------ the derived bound
GELU_TOL = {False: 3e-3, True: 2e-6}      # of max |ref|: tests/test_gpu_epilogue.py (gelu_fast against erf GELU)
DACT_TOL = {False: 3e-2, True: 1e-4}      # of max |ref|: tests/test_gpu_backward.py (the gradient chain through GELU')


def bound(d, rep: Replay, name: str) -> np.ndarray:
    """Largest |got - ref| the arithmetic of the contract allows per element of output ``name``.  Every fp16 x fp16 product is
    exact in fp32, so the sum carries at most Ktot roundings of 2^-24 relative to S; the split mode drops the lo x lo term
    (2^-22 S); bias, activation, derivative factor, residual and LeakyReLU copy are one fp32 rounding each (5 * 2^-24 |ref|);
    the store rounds to half an ulp of the output format (fp16: 2^-11, floor 2^-25; plane pair: 2^-22, floor 2^-25, the
    format's stated absolute error below 2^-14; fp32: 2^-24), applied to the value the kernel holds, i.e. ref + the error so far.
    gelu_fast and GELU' are approximations: the tolerances the suite already asserts for them are added where they are used."""
    ref, mask = rep.out[name]
    split = bool(d.split)
    e = (d.Ktot * 2.0 ** -24 + (2.0 ** -22 if split else 0.0)) * rep.S[name] * rep.amp[name]
    if d.act == ACT_GELU and name != "out_pre":
        e = e * 1.13                                      # max |GELU'|: the activation's Lipschitz constant
    e = e + 5 * 2.0 ** -24 * np.abs(ref)
    mx = float(np.abs(ref[mask]).max()) if mask.any() else 0.0
    if d.act == ACT_GELU and name != "out_pre":
        e = e + GELU_TOL[split] * mx
    if d.dact_src and name != "out_pre":
        e = e + DACT_TOL[split] * mx
    if name == "out_f":
        e = e + 2.0 ** -24 * (np.abs(ref) + e)
    elif split:
        e = e + np.maximum(2.0 ** -22 * (np.abs(ref) + e), 2.0 ** -25)
    else:
        e = e + np.maximum(2.0 ** -11 * (np.abs(ref) + e), 2.0 ** -25)
    return np.where(rep.zero[name], 0.0, e)


# ------------------------------------------------------------------------------------------------ the case table
SENTINEL_H, SENTINEL_F = 3.0, -7.0          # pre-fill of fp16-side / fp32 outputs (both planes of a pair hold SENTINEL_H)


@dataclass
class Case:
    """One entry of the table: light (the tensors are made on demand by ``spec``, seeded by the case, so every call gives the
    same data)."""
    inst: Instance
    name: str
    recipe: dict

    @property
    def id(self):
        return f"{self.inst.name}-{self.name}"

    def spec(self) -> "Spec":
        return _materialise(self.inst, self.name, **self.recipe)


@dataclass
class Spec:
    inst: Instance
    name: str
    plan_kw: dict                            # GemmPlan constructor arguments (without device)
    over: dict                               # descriptor fields set after construction
    ins: Dict[str, torch.Tensor]             # A0, A1: fp32 values (fp16-representable / split on demand) as flat tensors
    outs: Dict[str, int]                     # output name -> elements of one plane
    resid: Optional[str] = None              # None | "h" | "f" | "alias_h" (the output buffer is the residual) | "alias_f"
    dact: bool = False
    w_ld_slices: bool = False                # repack W [nz, rows, Kp] -> [rows, nz, Kp] (K-slices of one K-major matrix)

    @property
    def id(self):
        return f"{self.inst.name}-{self.name}"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _randn(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale).float()


def build_plan(case: Case, device=None) -> G.GemmPlan:
    """The case's plan through the ``GemmPlan`` constructor, the fields the constructor does not take set afterwards, the tile
    forced; ``plan.spec`` keeps the case's tensors for ``host_buffers``."""
    sp = case.spec()
    plan = G.GemmPlan(device=device, split=case.inst.split, **sp.plan_kw)
    plan.spec = sp
    d = plan.desc
    for k, v in sp.over.items():
        setattr(d, k, v)
    if sp.w_ld_slices:
        nz, Kp = d.nz, plan.Kp
        plan.w = plan.w.transpose(-3, -2).contiguous()
        d.w_ld, d.w_sZ = nz * Kp, Kp
    plan.tile = case.inst.tile
    return plan


def host_buffers(case: Case, plan: G.GemmPlan):
    """The launch's buffers on the host: ``bufs`` for ``replay`` (flat numpy), ``tens`` the same storage as torch tensors (to
    copy to a device), ``planes`` the plane length of every output, ``numel`` the total length of every buffer."""
    split = case.inst.split
    d = plan.desc
    case = plan.spec
    rng = _rng(case.id, "data")
    tens: Dict[str, torch.Tensor] = {}

    def h_side(x):                           # flat fp32 values -> the fp16-side storage (one plane, or hi | lo)
        x = x.reshape(-1)
        if split:
            return G.split_planes(x).reshape(-1)
        return x.half()

    for k in ("A0", "A1"):
        if k in case.ins:
            tens[k] = h_side(case.ins[k])
            if split:
                d.a_lo[int(k[1])] = case.ins[k].numel() // 8
    tens["W"] = plan.w.reshape(-1).cpu()
    if plan.bias is not None:
        tens["bias"] = plan.bias.reshape(-1).cpu()
    planes = dict(case.outs)
    plane_h = next((planes[o] for o in ("out_h", "out_h2", "out_pre") if o in planes), None)
    if plane_h is None and (case.dact or case.resid == "h"):
        plane_h = planes["out_f"]
    if split and plane_h is not None:
        d.o_lo = plane_h
    for o, n in case.outs.items():
        if o == "out_f":
            tens[o] = torch.full((n,), SENTINEL_F, dtype=torch.float32)
        else:
            assert n == plane_h, "fp16-side buffers of one launch share the plane length"
            tens[o] = torch.full((n * (2 if split else 1),), SENTINEL_H, dtype=torch.float16)
    first = "out_h" if "out_h" in planes else "out_f"
    if case.resid in ("h", "alias_h"):
        tens["resid"] = h_side(_randn(rng, plane_h))
        if case.resid == "alias_h":
            tens["out_h"] = tens["resid"]
    elif case.resid in ("f", "alias_f"):
        tens["resid"] = _randn(rng, planes[first])
        if case.resid == "alias_f":
            tens["out_f"] = tens["resid"]
    if case.dact:
        tens["dact_src"] = h_side(_randn(rng, plane_h, scale=1.5))
    bufs = {k: t.numpy() for k, t in tens.items()}
    bufs["ktab"] = plan.ktab_host
    numel = {k: int(t.numel()) for k, t in tens.items()}
    numel["ktab"] = len(plan.ktab_host)
    d.resid_f32 = int(case.resid in ("f", "alias_f"))
    return bufs, tens, planes, numel


def case_desc(case: Case, plan: G.GemmPlan):
    """``desc_fields`` with the pointer flags a launch of this case sets."""
    d = desc_fields(plan.desc)
    case = plan.spec
    d.A0, d.A1, d.W, d.ktab = True, "A1" in case.ins, True, True
    d.bias = plan.bias is not None
    d.resid = case.resid is not None
    d.dact_src = case.dact
    for o in OUTS:
        setattr(d, o, o in case.outs)
    return d


def _ndiv_for(N):
    """A column-block width (% 4, or % 8 when N % 8 == 0) that cuts N into an odd number >= 3 of blocks."""
    step = 8 if N % 8 == 0 else 4
    for nd in range(N // 3 // step * step, 0, -step):
        if N % nd == 0 and (N // nd) % 2 == 1:
            return nd
    raise AssertionError(N)


def _gather_case(inst: Instance, name: str, **recipe) -> Case:
    return Case(inst, name, recipe)


def _materialise(inst: Instance, name: str, *, wide=True, tiles_n=2, two_src=False, halo_zero=True, act="none", bias=True,
                 outs=("out_h",), resid=None, dact=False, nz=1, nz_lo=0, z_inner=False, sc=0, ndiv=False, nsub=False,
                 phase=False, w_ld=False, affine=False, plain_out=False) -> Spec:
    """A convolution-like launch: rows enumerate a (B, Hg, Wg) grid whose window leaves a one-row, one-column halo, 17 real
    K chunks (3 x 3 taps over a 2-chunk pixel minus one, or 9 + 8 over two sources) padded to Ktot = 192.
    ``affine``: the Linear / Conv1d-like geometry of ``desc.plain`` instead (identity K table, overlapping rows of 18 chunks pitch)."""
    BM, BN = inst.BM, inst.BN
    N = (tiles_n - 1) * BN + (8 if wide else 4)
    rng = _rng(inst.BM, inst.BN, inst.split, name, "w")
    B, Hg, Wg = (3, 7, 13) if BM == 128 else (3, 11, 17)
    nzh = nz // nz_lo if nz_lo > 1 else nz
    ins = {}
    if affine:
        Hg, Wg = 1, (2 * BM + 17 + 2) // 3
        M = B * Hg * Wg
        pitch = 18                                            # chunks between rows: rows overlap (K = 17 real chunks, 24 read)
        window = (0, 1, 0, Wg) if plain_out else (0, 1, 1, Wg - 1)
        ktab = np.arange(24, dtype=np.int64)                  # identity table: the 7 padding chunks are real reads of zero weights
        zs, zs2 = (3 if nz > 1 else 0), (1 if nz_lo > 1 else 0)       # batches shift the rows by 3 chunks (and 1 at the low level)
        sources = [G.Source(Hg * Wg * pitch, 0, pitch, 0, sZ=zs, sZ2=zs2)]
        ins["A0"] = _randn(rng, ((M - 1) * pitch + 24 + zs * (nzh - 1) + zs2) * 8)
    else:
        M = B * Hg * Wg
        window = (1, Hg - 1, 1, Wg - 1)
        Hs, Ws = Hg + 1, Wg + 1                               # one spare row / column for the batch shifts a_sZ / a_sZ2
        taps = (np.arange(3)[:, None] * Ws + np.arange(3)[None, :]).reshape(-1)
        if two_src:
            ktab = np.concatenate([taps, taps[:8] | (1 << 31)]).astype(np.int64)
            ccs = (1, 1)
        else:
            ktab = (taps[:, None] * 2 + np.arange(2)[None, :]).reshape(-1)[:17].astype(np.int64)
            ccs = (2,)
        sources = []
        for s, cc in enumerate(ccs):
            sources.append(G.Source(Hs * Ws * cc, Ws * cc, cc, -(Ws + 1) * cc, sZ=Ws * cc if nz > 1 else 0, sZ2=cc if nz_lo > 1 else 0))
            ins["A%d" % s] = _randn(rng, (B * Hs * Ws + (nzh - 1) * Ws) * cc * 8)
    K = 8 * len(ktab)
    w2 = _randn(rng, nz, N, K, scale=136 ** -0.5)
    w2[:, :, 136:] = 0.0
    bias_t = _randn(rng, nz * N) if bias else None
    step = 8 if wide else 4
    Ct = N + 2 * step                                         # channel pitch: a sentinel slice on both sides of the N columns
    kw = dict(M=M, N=N, w2=w2, ktab=ktab, sources=sources, Hg=Hg, Wg=Wg, window=window, halo_zero=halo_zero and not plain_out,
              bias=bias_t, bias_sZ=N if (bias and nz > 1) else 0, act=act, slope=0.2, slope2=0.1, nz=nz, nz_lo=nz_lo, z_inner=z_inner,
              plain=affine)
    if ndiv or nsub or phase:
        nd = _ndiv_for(N)
        Q = N // nd
        cp = nd + step                                        # pitch of one column block
        if phase:                                             # block q = output phase: position t = w * Q + q - pad, cut at both ends
            pad = Q + 1                                       # first window column: phase 0 falls before the line
            T = (Wg - 2) * Q + Q - 1 - pad                    # last window column: the last phase falls behind it
            line = (T + 4) * cp
            kw.update(out=(Hg * line, line, Q * cp, (2 - pad) * cp + step), n_div=nd, o_sNhi=cp, phase=(Q, pad, T))
            plane = B * Hg * line
        elif nsub:                                            # blocks q -> (q // 2) * o_sNhh + (q % 2) * o_sNhi
            hh = 2 * cp + step
            pix = (Q + 1) // 2 * hh
            kw.update(out=(Hg * Wg * pix, Wg * pix, pix, step), n_div=nd, o_sNhi=cp, n_sub=2, o_sNhh=hh)
            plane = B * Hg * Wg * pix + step
        else:
            pix = Q * cp
            kw.update(out=(Hg * Wg * pix, Wg * pix, pix, step), n_div=nd, o_sNhi=cp)
            plane = B * Hg * Wg * pix + step
    else:
        kw.update(out=(Hg * Wg * Ct, Wg * Ct, Ct, step))
        plane = M * Ct
    if nz > 1:
        kw.update(o_sZ=plane * (nz_lo if nz_lo > 1 else 1), o_sZ2=plane if nz_lo > 1 else 0)
        plane *= nz
    over = {"sc": sc}
    return Spec(inst, name, kw, over, ins, {o: plane for o in outs}, resid=resid, dact=dact, w_ld_slices=w_ld)


def _row_recipes(inst: Instance, affine: bool) -> List[Case]:
    a = dict(affine=affine)
    pre = "arow_" if affine else "row_"
    c = [
        _gather_case(inst, pre + "none_nohalo", act="none", bias=False, halo_zero=False, **a),
        _gather_case(inst, pre + "none", act="none", **a),
        _gather_case(inst, pre + "gelu", act="gelu", **a),
        _gather_case(inst, pre + "leaky", act="leaky", **a),
        _gather_case(inst, pre + "resid_h2", resid="h", outs=("out_h", "out_h2"), **a),
        _gather_case(inst, pre + "outf", outs=("out_f",), act="leaky", **a),
        _gather_case(inst, pre + "ndiv_narrow", wide=False, ndiv=True, act="leaky", **a),
    ]
    if affine:
        return c + [
            _gather_case(inst, "arow_nsub", nsub=True, halo_zero=False, **a),
            _gather_case(inst, "arow_phase", phase=True, halo_zero=False, **a),
            _gather_case(inst, "arow_wld_slices", outs=("out_f",), nz=4, w_ld=True, bias=False, halo_zero=False, **a),
            _gather_case(inst, "arow_z", tiles_n=3, nz=4, nz_lo=2, act="leaky", **a),
            _gather_case(inst, "arow_z_inner", tiles_n=3, nz=4, nz_lo=2, z_inner=True, act="leaky", **a),
        ]
    c += [
        _gather_case(inst, "row_resid_h", resid="h"),
        _gather_case(inst, "row_h2", outs=("out_h", "out_h2")),
        _gather_case(inst, "row_resid_alias", resid="alias_h"),
        _gather_case(inst, "row_resid_f32", resid="f"),
        _gather_case(inst, "row_pre", act="gelu", outs=("out_h", "out_pre")),
        _gather_case(inst, "row_dact", dact=True, halo_zero=False),
        _gather_case(inst, "row_narrow", wide=False, act="gelu"),
        _gather_case(inst, "row_ndiv_wide", ndiv=True, halo_zero=False),
        _gather_case(inst, "row_nsub", nsub=True, halo_zero=False),
        _gather_case(inst, "row_phase", phase=True, halo_zero=False),
        _gather_case(inst, "row_two_src", two_src=True, act="leaky"),
        _gather_case(inst, "row_wld_slices", outs=("out_f",), nz=4, w_ld=True, bias=False, halo_zero=False),
        _gather_case(inst, "row_z", tiles_n=3, nz=4, nz_lo=2, act="leaky", two_src=True),
        _gather_case(inst, "row_z_inner", tiles_n=3, nz=4, nz_lo=2, z_inner=True, act="leaky", two_src=True),
        _gather_case(inst, "row_sc", tiles_n=3, sc=2, halo_zero=False),
    ]
    return c


def _plain_recipes(inst: Instance) -> List[Case]:
    a = dict(affine=True, plain_out=True)
    return [
        _gather_case(inst, "plain_none", **a),
        _gather_case(inst, "plain_none_nobias", bias=False, **a),
        _gather_case(inst, "plain_gelu", act="gelu", **a),
        _gather_case(inst, "plain_leaky", act="leaky", **a),
        _gather_case(inst, "plain_f32_resid", outs=("out_f",), resid="alias_f", **a),
        _gather_case(inst, "plain_resid_h", resid="h", **a),
        _gather_case(inst, "plain_h2", outs=("out_h", "out_h2"), **a),
        _gather_case(inst, "plain_h_and_f", outs=("out_h", "out_f"), **a),
        _gather_case(inst, "plain_narrow", wide=False, act="gelu", **a),
        _gather_case(inst, "plain_z", nz=2, tiles_n=3, sc=2, **a),
    ]


def _cases() -> List[Case]:
    out: List[Case] = []
    for inst in INSTANCES.values():
        if inst.plain is not True:
            out += _row_recipes(inst, affine=False)
        if inst.plain is not False:
            out += _plain_recipes(inst) + _row_recipes(inst, affine=True)
        elif not (inst.tile == G.TILE_128x128):
            # desc.plain on a tile without an affine loader: the gathered loader serves it (a_sB / a_sH consistent with a_sW)
            out += [_gather_case(inst, "plainflag_none", affine=True, plain_out=True),
                    _gather_case(inst, "plainflag_rows_leaky", affine=True, act="leaky")]
    return out


CASES: List[Case] = _cases()
CASE_IDS = [c.id for c in CASES]


def features(inst: Instance, d) -> set:
    """The addressing features of include/addvisor_hip.h a launch of ``d`` on ``inst`` exercises."""
    tilesM, tilesN = -(-d.M // inst.BM), -(-d.N // inst.BN)
    nz = max(d.nz, 1)
    f = {"padding_chunks"}
    if d.A1:
        f.add("two_sources")
    if d.halo_zero:
        f.add("halo_zero")
    if (d.h0, d.h1, d.w0, d.w1) != (0, d.Hg, 0, d.Wg):
        f.add("window")
    if nz > 1:
        f.add("nz")
    if d.nz_lo > 1:
        f.add("nz_lo")
    if d.z_inner:
        f.add("z_inner")
    if (tilesM * tilesN * (nz if d.z_inner else 1)) % 8:
        f.add("remap_remainder")
    if 0 < d.sc < tilesN and tilesN % d.sc:
        f.add("sc_ragged")
    if d.w_ld not in (0, d.Ktot):
        f.add("w_ld")
    if d.n_div < d.N:
        f.add("n_div")
    if d.n_sub > 1:
        f.add("n_sub")
    if d.ph_r > 0:
        f.add("phase")
    if d.M % inst.BM and tilesM >= 3:
        f.add("ragged_m")
    if d.N % inst.BN and tilesN >= 2:
        f.add("ragged_n")
    return f


# ------------------------------------------------------------------------------------------------ single mutations
def mutations(d) -> List[Tuple[str, Callable]]:
    """The single mistakes of the issue's list that apply to descriptor ``d`` (a mutation of a field the launch does not use
    cannot change anything and is not listed), as (name, function mutating a copy of ``d``; returns replay keyword arguments)."""
    out = []

    def add(name, fn):
        out.append((name, fn))

    if d.n_sub > 1:
        def f(x):
            x.o_sNhi, x.o_sNhh = x.o_sNhh, x.o_sNhi
        add("o_sNhi<->o_sNhh", f)
    for fld, dv in (("h0", 1), ("h1", -1), ("w0", 1), ("w1", -1)):
        lo, hi = (d.h0, d.h1) if fld[0] == "h" else (d.w0, d.w1)
        if hi - lo >= 2:
            add(f"{fld}{dv:+d}", lambda x, fld=fld, dv=dv: setattr(x, fld, getattr(x, fld) + dv))
    if d.A1:
        add("bit31_cleared", "ktab")
    if d.nz_lo > 1:
        def f(x):
            x.a_sZ, x.a_sZ2 = x.a_sZ2, x.a_sZ
        add("a_sZ<->a_sZ2", f)
    if d.w_ld not in (0, d.Ktot):
        add("w_ld->Ktot", lambda x: setattr(x, "w_ld", x.Ktot))
    if d.ph_r > 0:
        add("ph_pad+1", lambda x: setattr(x, "ph_pad", x.ph_pad + 1))
        add("ph_pad-1", lambda x: setattr(x, "ph_pad", x.ph_pad - 1))
    if max(d.nz, 1) > 1 and d.bias and d.bias_sZ:
        add("bias_sZ->0", lambda x: setattr(x, "bias_sZ", 0))
    if d.out_h2:
        add("slope2->slope", lambda x: setattr(x, "slope2", x.slope))
    if d.wide:
        add("drop_wide_permutation", "drop_wide")
    if d.split:                                         # beyond the issue's list: the split bound must still see a lost lo plane
        add("A_lo_planes_dropped", "lo_A")
        add("W_lo_plane_dropped", "lo_W")
    return out
