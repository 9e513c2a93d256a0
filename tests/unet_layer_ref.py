"""fp64 definitions of the inference U-Net's layers, readers for its feature maps and the elementwise error bound that
tests/test_gpu_unet_layers.py and tests/test_gpu_unet_f16_tiles.py hold the HIP kernels to (pinned on the CPU by
tests/test_unet_layer_ref_cpu.py).

The references are plain torch on NCHW fp64 tensors, written from addvisor.py:12-84 as oracle/unet_ref.py is: a convolution is
``F.conv2d``, a transposed convolution ``F.conv_transpose2d``, and the fused stage is those two one after the other.  None of them
knows a plan, a descriptor, a composed weight or a packing.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

SLOPE = 0.2
BN_EPS = 1e-5

# destination map -> (convolution, its BatchNorm, stride, padding, dilation): addvisor.py:31-54
CONVS = {
    "x1a": ("e1.block.0", "e1.block.1", (2, 1), (2, 1), (1, 1)), "x1": ("e1.block.3", "e1.block.4", (1, 1), (1, 1), (1, 1)),
    "x2a": ("e2.block.0", "e2.block.1", (2, 1), (2, 1), (1, 1)), "x2": ("e2.block.3", "e2.block.4", (1, 1), (1, 1), (1, 1)),
    "x3a": ("e3.block.0", "e3.block.1", (2, 2), (1, 1), (1, 1)), "x3": ("e3.block.3", "e3.block.4", (1, 1), (1, 1), (1, 1)),
    "x4a": ("e4.block.0", "e4.block.1", (2, 2), (1, 1), (1, 1)), "x4": ("e4.block.3", "e4.block.4", (1, 1), (1, 1), (1, 1)),
    "b1": ("bottleneck.0", "bottleneck.1", (1, 1), (2, 2), (2, 2)), "b2": ("bottleneck.3", "bottleneck.4", (1, 1), (4, 4), (4, 4)),
    "y4a": ("d4.block.0", "d4.block.1", (1, 1), (1, 1), (1, 1)), "y4": ("d4.block.3", "d4.block.4", (1, 1), (1, 1), (1, 1)),
    "y3a": ("d3.block.0", "d3.block.1", (1, 1), (1, 1), (1, 1)), "y3": ("d3.block.3", "d3.block.4", (1, 1), (1, 1), (1, 1)),
    "y2a": ("d2.block.0", "d2.block.1", (1, 1), (1, 1), (1, 1)), "y2": ("d2.block.3", "d2.block.4", (1, 1), (1, 1), (1, 1)),
    "y1a": ("d1.block.0", "d1.block.1", (1, 1), (1, 1), (1, 1)), "y1": ("d1.block.3", "d1.block.4", (1, 1), (1, 1), (1, 1)),
}
# decoder stages: (coarse map, up-sampled map, skip map, first map of the block, its output, ConvTranspose2d, stride)
STAGES = [("b2", "u4", "x3", "y4a", "y4", "up4", (2, 2)), ("y4", "u3", "x2", "y3a", "y3", "up3", (2, 2)),
          ("y3", "u2", "x1", "y2a", "y2", "up2", (2, 1)), ("y2", "u1", "x", "y1a", "y1", "up1", (2, 1))]
UPS = {u: (up, stride) for _, u, _, _, _, up, stride in STAGES}            # up-sampled map -> (ConvTranspose2d, stride)
STAGE_OF = {mid: (up, stride) for _, _, _, mid, _, up, stride in STAGES}    # first map of a decoder block -> its ConvTranspose2d


# ------------------------------------------------------------------------------------------------ the layers
def conv_layer(srcs, w, b, stride=(1, 1), padding=(1, 1), dilation=(1, 1), slope=SLOPE):
    """``leaky_relu(conv2d(cat(srcs), w) + b)``; ``slope=None``: no activation."""
    y = F.conv2d(torch.cat(list(srcs), 1), w, b, stride=stride, padding=padding, dilation=dilation)
    return y if slope is None else F.leaky_relu(y, slope)


def convT_layer(src, wt, bt, stride):
    """nn.ConvTranspose2d with kernel == stride (addvisor.py:45-54)."""
    assert tuple(wt.shape[2:]) == tuple(stride)
    return F.conv_transpose2d(src, wt, bt, stride=stride)


def upconv_layer(coarse, skip, wt, bt, wc, bc, stride, slope=SLOPE):
    """``leaky_relu(conv2d(cat([convT(coarse) + bt, skip]), wc, padding=1) + bc)``, layer by layer."""
    u = convT_layer(coarse, wt, None, stride) + bt.view(1, -1, 1, 1)
    return conv_layer([u, skip], wc, bc, slope=slope)


def fold_bn(sd, conv: str, bn: str):
    """Eval-mode BatchNorm folded into its convolution, in fp64: ``(w, b, |b| bound)``.  The third value is the fold evaluated on
    absolute values, ``(|b| + |mean|) |s| + |beta|``: what a fold in fp32 rounds relative to, and the bias ``bound``'s ``A`` takes."""
    d = lambda k: sd[k].detach().cpu().double()
    s = d(bn + ".weight") / torch.sqrt(d(bn + ".running_var") + BN_EPS)
    w, b = d(conv + ".weight"), d(conv + ".bias")
    return (w * s.view(-1, 1, 1, 1), (b - d(bn + ".running_mean")) * s + d(bn + ".bias"),
            (b.abs() + d(bn + ".running_mean").abs()) * s.abs() + d(bn + ".bias").abs())


def unet_chain(x, sd, conv, convT, stage=None):
    """The whole network (addvisor.py:62-84) as a chain of layer calls on ``x [B, 1, H, W]`` fp64; returns ``(logits, mask)``.
    ``conv(dst, srcs, w, b, ab, stride, padding, dilation)``, ``convT(dst, src, wt, bt, stride)`` and -- if given, in place of a
    stage's ``convT`` + first ``conv`` -- ``stage(dst, coarse, skip, wt, bt, wc, bc, abc, stride)`` each return the map ``dst``."""
    d = lambda k: sd[k].detach().cpu().double()

    def c(dst, srcs):
        cn, bn, st, pd, dl = CONVS[dst]
        return conv(dst, srcs, *fold_bn(sd, cn, bn), st, pd, dl)

    m = {"x": x}
    m["x1"] = c("x1", [c("x1a", [x])])
    for a, o, i in (("x2a", "x2", "x1"), ("x3a", "x3", "x2"), ("x4a", "x4", "x3")):
        m[o] = c(o, [c(a, [m[i]])])
    m["b2"] = c("b2", [c("b1", [m["x4"]])])
    for coarse, u, skip, mid, out, up, stride in STAGES:
        wt, bt = d(up + ".weight"), d(up + ".bias")
        if stage is None:
            ya = c(mid, [convT(u, m[coarse], wt, bt, stride), m[skip]])
        else:
            ya = stage(mid, m[coarse], m[skip], wt, bt, *fold_bn(sd, *CONVS[mid][:2]), stride)
        m[out] = c(out, [ya])
    logits = head(m["y1"], d("mask_head.0.weight"), d("mask_head.0.bias"))
    return logits, torch.sigmoid(logits)


def head(y1, hw, hb):
    """The 1x1 mask head (addvisor.py:57-60) before its sigmoid."""
    return F.conv2d(y1, hw.reshape(1, -1, 1, 1), hb.reshape(1))


# ------------------------------------------------------------------------------------------------ map readers
def read_map(f, channels=None) -> torch.Tensor:
    """Interior of an ``FMap`` as NCHW fp64 on the CPU; a split-format plane pair is joined as ``hi + lo * 2^-11`` (exact in
    fp64).  ``channels``: the first that many (a fused coarse map carries an indicator chunk and padding channels behind its real
    ones, the unfused ``u1`` the packed spectrogram chunk) or a slice."""
    t = f.t.detach().cpu().double()
    t = t[0] + t[1] * 2.0 ** -11 if f.split else t
    t = t[:, f.PH:f.PH + f.H, f.PW:f.PW + f.W, :]
    if channels is not None:
        t = t[..., channels if isinstance(channels, slice) else slice(0, channels)]
    return t.permute(0, 3, 1, 2).contiguous()


def read_halo(f) -> torch.Tensor:
    """Every stored element of an ``FMap`` outside its interior (both planes in split mode), as stored: fp16
    ``[(2,) B, halo pixels, C]``."""
    t = f.t.detach().cpu()
    outside = torch.ones(f.Hp, f.Wp, dtype=torch.bool)
    outside[f.PH:f.PH + f.H, f.PW:f.PW + f.W] = False
    return t[..., outside, :]


def to_nhwc(x, dtype=torch.float16):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


# ------------------------------------------------------------------------------------------------ the bound
def bound(ref, A, K: int, mode: str, out: str = "map", operands: str = "rounded"):
    """Largest ``|got - ref|`` the arithmetic allows per element, in the form of ``gemm_desc_ref.bound``.

    ``ref``: the layer in fp64 on the operands the kernel read; ``A``: the same layer on ``|inputs|``, ``|weights|``, ``|biases|`` (for
    the fused stage layer by layer on absolute values, which bounds ``sum |W_composed| |x|`` by the triangle inequality);
    ``K``: the reduction length; ``mode``: "f16" | "split".

    fp16:  ``e = (K 2^-24 + 2^-11) A + 5 2^-24 |ref|`` -- fp32 accumulation of exact fp16 x fp16 products (at most K roundings
    relative to the running sum, itself at most A), the fp16 rounding of the folded / composed weights, which the reference does
    not apply (half an ulp, 2^-11, of every term), and one fp32 rounding each for bias, slope, ... -- then the store, half an ulp of
    the value the kernel holds: ``e + max(2^-11 (|ref| + e), 2^-25)`` (2^-25: half the smallest fp16 subnormal).
    split: 2^-22 in place of 2^-11 in both places (a plane pair keeps 22 bits), plus the lo x lo products the three-MFMA form drops,
    ``2^-22 A``.
    ``out="f32"``: the value is stored as fp32 (the head's logits): the store term is ``2^-24 (|ref| + e)``.
    ``operands="exact"``: a direct kernel that multiplies fp32 weights with the values it read in plain fp32 (stem, pack, head): no
    operand is rounded to the map format and no lo x lo product is dropped, so both of those terms go; what such a kernel rounds
    besides its K multiply-adds (the fp32 BatchNorm fold of its weights, the join of a plane pair) is counted into ``K``."""
    assert mode in ("f16", "split") and out in ("map", "f32") and operands in ("rounded", "exact")
    u = 2.0 ** -11 if mode == "f16" else 2.0 ** -22
    ref, A = ref.abs(), A.abs()
    ops = 0.0 if operands == "exact" else u + (2.0 ** -22 if mode == "split" else 0.0)
    e = (K * 2.0 ** -24 + ops) * A + 5 * 2.0 ** -24 * ref
    if out == "f32":
        return e + 2.0 ** -24 * (ref + e)
    return e + torch.clamp(u * (ref + e), min=2.0 ** -25)


def sigmoid_bound(e_logit):
    """``|sigmoid(a') - sigmoid(a)|`` for ``|a' - a| <= e_logit`` evaluated in fp32: the sigmoid's slope is at most 1/4, and ``expf``
    (2 ulp), the addition and the division (half an ulp each, correctly rounded) move a result of at most 1 by less than
    4 * 2^-24; the fp64 reference's own sigmoid is exact to 2^-52."""
    return e_logit / 4 + 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ CPU models of the kernels
def _split(x):
    """``gemm.split_planes`` / its exact fp64 join."""
    from addvisor_hip import gemm as G
    p = G.split_planes(x)
    return p, p[0].double() + p[1].double() * 2.0 ** -11


def store(y32, mode):
    """An fp32 value as the map holds it (fp64)."""
    return y32.half().double() if mode == "f16" else _split(y32.double())[1]


def as_stored(x, mode):
    """Any fp64 tensor rounded to values a map of that mode can hold."""
    return x.half().double() if mode == "f16" else _split(x)[1]


def model_conv(srcs, w, b, stride=(1, 1), padding=(1, 1), dilation=(1, 1), slope=SLOPE, mode="f16"):
    """What a kernel of the contract computes for ``conv_layer``: fp16 operands (weights rounded, inputs as stored), products summed in
    fp32, fp32 bias and LeakyReLU, fp16 store; split: the three fp16 plane products hi hi + (hi lo + lo hi) 2^-11 summed in fp32 and
    a plane-pair store."""
    x = torch.cat(list(srcs), 1)
    geom = dict(stride=stride, padding=padding, dilation=dilation)
    if mode == "f16":
        assert torch.equal(x, x.half().double())
        y = F.conv2d(x.float(), w.half().float(), None, **geom)
    else:
        (xs, xj), (ws, _) = _split(x), _split(w)
        assert torch.equal(x, xj)
        y = F.conv2d(xs[0].float(), ws[0].float(), None, **geom) + \
            (F.conv2d(xs[0].float(), ws[1].float(), None, **geom) + F.conv2d(xs[1].float(), ws[0].float(), None, **geom)) * 2.0 ** -11
    if b is not None:
        y = y + b.float().view(1, -1, 1, 1)
    return store(y if slope is None else F.leaky_relu(y, slope), mode)


def model_convT(src, wt, bt, stride, mode="f16"):
    geom = dict(stride=stride)
    if mode == "f16":
        y = F.conv_transpose2d(src.float(), wt.half().float(), None, **geom)
    else:
        (xs, _), (ws, _) = _split(src), _split(wt)
        y = F.conv_transpose2d(xs[0].float(), ws[0].float(), None, **geom) + \
            (F.conv_transpose2d(xs[0].float(), ws[1].float(), None, **geom)
             + F.conv_transpose2d(xs[1].float(), ws[0].float(), None, **geom)) * 2.0 ** -11
    return store(y + bt.float().view(1, -1, 1, 1), mode)


def model_upconv(coarse, skip, wt, bt, wc, bc, stride, slope=SLOPE, mode="f16", indicator="skip", exact=False):
    """The fused stage as the kernels run it: ``gemm.compose_upconv_weights`` (fp64) rounded to the operand format, one small
    convolution over the coarse map per output parity class plus the 3 x 3 taps of the skip map, the transposed convolution's bias
    through the in-image indicator channel.  ``exact``: no rounding anywhere (fp64): must then equal ``upconv_layer``."""
    from addvisor_hip import gemm as G
    sh, sw = stride
    Cb, Cs, N = wt.shape[0], skip.shape[1], wc.shape[0]
    B, _, Hc, Wc = coarse.shape
    one = torch.ones(B, 1, Hc, Wc, dtype=torch.float64)
    pad8 = lambda t: torch.cat([t, t.new_zeros(B, -t.shape[1] % 8, *t.shape[2:])], 1)
    if indicator == "coarse":                                              # the indicator opens the chunk behind the real channels
        xc, xs, ich = pad8(torch.cat([coarse, one], 1)), pad8(skip), Cb
    else:
        xc, xs, ich = pad8(coarse), pad8(torch.cat([skip, torch.ones(B, 1, sh * Hc, sw * Wc, dtype=torch.float64)], 1)), Cs
    w2, cu0, cu1 = G.compose_upconv_weights(wt, bt, wc, stride, (indicator, ich))
    assert xc.shape[1] == cu0 * 8 and xs.shape[1] == cu1 * 8
    nth, ntw = 2, (2 if sw == 2 else 3)
    xcp = F.pad(xc, (1, 1, 1, 1))

    def conv3(x, w, **kw):                                                 # x as stored, w fp64
        if exact:
            return F.conv2d(x, w, None, **kw)
        if mode == "f16":
            return F.conv2d(x.float(), w.half().float(), None, **kw)
        (xp, _), (wp, _) = _split(x), _split(w)
        return F.conv2d(xp[0].float(), wp[0].float(), None, **kw) + \
            (F.conv2d(xp[0].float(), wp[1].float(), None, **kw) + F.conv2d(xp[1].float(), wp[0].float(), None, **kw)) * 2.0 ** -11

    y = torch.zeros(B, N, sh * Hc, sw * Wc, dtype=torch.float64 if exact else torch.float32)
    for ph in range(sh):
        for pw in range(sw):
            w = w2[ph * sw + pw]
            k0 = nth * ntw * cu0 * 8
            w0 = w[:, :k0].reshape(N, nth, ntw, cu0 * 8).permute(0, 3, 1, 2)
            w1 = w[:, k0:].reshape(N, 3, 3, cu1 * 8).permute(0, 3, 1, 2)
            r0, c0 = 1 + (ph - 1) // sh, 1 + (pw - 1) // sw               # first coarse tap of this parity in the padded map
            part = conv3(xcp[:, :, r0:r0 + Hc + nth - 1, c0:c0 + Wc + ntw - 1].contiguous(), w0)
            y[:, :, ph::sh, pw::sw] = part + conv3(xs, w1, padding=1)[:, :, ph::sh, pw::sw]
    y = y + (bc.view(1, -1, 1, 1) if exact else bc.float().view(1, -1, 1, 1))
    y = y if slope is None else F.leaky_relu(y, slope)
    return y if exact else store(y, mode)


# ------------------------------------------------------------------------------------------------ the line tiles' direct cases
# advh_conv53s21_tile_f16, (B, Ho, W, (source halo, destination halo)); the tile is 8 x 16 and the grid at most 256 workgroups:
# 416 tiles (160 workgroups walk a second one), 520 tiles (8 workgroups a third: the patch buffer index returns to 0), then ragged
# heights / widths and other halos
P1_S21 = ((2, 1), (1, 1))
S21_CASES = [(2, 128, 196, P1_S21), (5, 64, 200, P1_S21), (1, 1, 1, P1_S21), (3, 5, 15, P1_S21), (1, 17, 33, ((3, 2), (1, 1))),
             (3, 16, 50, ((2, 1), (2, 3))), (1, 40, 15, ((4, 4), (0, 0))), (1, 1, 50, P1_S21), (2, 33, 16, P1_S21)]
# advh_upconv21_tile_f16, (B, Hc, W, (coarse, skip, destination halo)), Hc % 8 == 0; 16 x 16 output tiles: 520 tiles, the production
# geometry (416 tiles), then ragged widths and other halos
P1_UP = ((1, 1), (1, 1), (1, 1))
UPCONV_CASES = [(5, 64, 200, P1_UP), (2, 256, 196, P1_UP), (1, 8, 1, P1_UP), (3, 8, 15, P1_UP), (1, 16, 33, ((2, 1), (1, 2), (1, 1))),
                (3, 16, 50, ((1, 2), (2, 1), (2, 3))), (1, 40, 15, P1_UP), (1, 8, 50, P1_UP)]
# advh_conv_taps2d_f16, (Cn, B, H, W, PH, PW); 16 x 16 tiles: 546 tiles > the 32-channel grid of 512, 270 > the 64-channel grid of 256,
# then the four shapes of tests/test_gpu_gemm.py::test_conv2d_line_tile
TAPS2D_CASES = [(32, 3, 208, 224, 1, 1), (64, 2, 144, 240, 1, 1), (32, 2, 37, 50, 2, 1), (64, 3, 16, 16, 1, 1), (64, 1, 70, 33, 1, 2),
                (32, 1, 256, 196, 1, 1)]


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def s21_data(B, Ho, W, mode="f16"):
    """e2.block.0-shaped operands: ``(x [B, 32, 2 Ho, W] as stored, w [64, 32, 5, 3], b [64])``."""
    g = torch.Generator().manual_seed(31 * B + 7 * Ho + W)
    return as_stored(_randn(g, B, 32, 2 * Ho, W), mode), _randn(g, 64, 32, 5, 3) / (15 * 32) ** 0.5, _randn(g, 64) * 0.1


def upconv_data(B, Hc, W, mode="f16"):
    """up1 + d1.block.0-shaped operands: coarse ``[B, 64, Hc, W]`` and the spectrogram channel ``[B, 1, 2 Hc, W]`` as stored, then
    ``wt, bt, wc, bc``.  The transposed convolution's bias is scaled x8 so that the indicator path carries weight."""
    g = torch.Generator().manual_seed(77 * B + Hc + W)
    xc, xs = as_stored(_randn(g, B, 64, Hc, W), mode), as_stored(torch.rand(B, 1, 2 * Hc, W, generator=g, dtype=torch.float64) * 3, mode)
    return (xc, xs, _randn(g, 64, 32, 2, 1) / 8, _randn(g, 32) * 0.1 * 8, _randn(g, 32, 33, 3, 3) / (3 * 33 ** 0.5), _randn(g, 32) * 0.1)


def taps2d_data(Cn, B, H, W, mode="f16"):
    g = torch.Generator().manual_seed(Cn + H)
    return as_stored(_randn(g, B, Cn, H, W), mode), _randn(g, Cn, Cn, 3, 3) / (3 * Cn ** 0.5), _randn(g, Cn)


# direct kernels (``bound(..., operands="exact")``): 15 multiply-adds + the fp32 BatchNorm fold of the weights (rsqrt of var + eps, the
# scale, its product with the weight: 5 roundings); 32 multiply-adds + the join of a plane pair + two shuffle additions
K_STEM, K_HEAD = 20, 35
K_S21, K_UPCONV = 480, 480             # 15 taps x 32 channels; the composed K of 456 zero-padded to 15 k-steps of 32
S21_GEOM = dict(stride=(2, 1), padding=(2, 1))
