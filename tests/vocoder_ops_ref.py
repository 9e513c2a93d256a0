"""fp64 restatement of the HiFi-GAN vocoder's operations, for the kernel-level tests (tests/test_gpu_vocoder_kernels.py).

Plain torch, written from the formulas of the published V1 generator (Kong et al. 2020) -- sums over taps, not
``torch.nn.functional`` convolutions and not the kernels.  Values are channels-last ``[B, T, C]`` like the HIP maps; weights keep
torch's layouts (Conv1d ``[Cout, Cin, k]``, ConvTranspose1d ``[Cin, Cout, k]``).  Every function computes in float64 whatever dtype it
is handed, except ``halo_fill`` and ``pack_mel``, which only move values and keep the dtype.  tests/test_vocoder_ops_ref_cpu.py pins
each helper against ``torch.nn.functional`` and the composed generator against oracle/hifigan_ref.py.
"""
import torch


def lrelu(x, slope):
    x = x.double()
    return torch.where(x > 0, x, x * slope)


def conv1d_same(x, w, b, dilation=1, padded=None):
    """Conv1d with "same" padding (k - 1) * dilation / 2: ``y[t] = b + sum_j xp[t + j * dilation] @ w[:, :, j].T``.
    ``x [B, T, Cin]`` is zero-padded, unless ``padded [B, T + 2 * halo, Cin]`` is given: then the taps read that map, whatever
    its halo rows hold (halo >= the padding), and ``x`` only states T."""
    Cout, Cin, k = w.shape
    pad = (k - 1) * dilation // 2
    B, T = x.shape[0], x.shape[1]
    if padded is None:
        xp = torch.zeros(B, T + 2 * pad, Cin, dtype=torch.float64)
        xp[:, pad:pad + T] = x.double()
    else:
        halo = (padded.shape[1] - T) // 2
        assert padded.shape[1] == T + 2 * halo and halo >= pad
        xp = padded.double()[:, halo - pad:halo + T + pad]
    y = torch.zeros(B, T, Cout, dtype=torch.float64)
    for j in range(k):
        y += xp[:, j * dilation:j * dilation + T] @ w[:, :, j].double().T
    return y if b is None else y + b.double()


def conv_transpose1d(x, w, b, stride):
    """ConvTranspose1d(k = 2 * stride, stride, padding = stride / 2): input q adds ``x[q] @ w[:, :, j]`` to output
    ``q * stride + j - padding``.  ``x [B, T, Cin]``, ``w [Cin, Cout, k]`` -> ``[B, T * stride, Cout]``."""
    Cin, Cout, k = w.shape
    assert k == 2 * stride and stride % 2 == 0
    pad = stride // 2
    B, T = x.shape[0], x.shape[1]
    full = torch.zeros(B, (T - 1) * stride + k, Cout, dtype=torch.float64)
    for j in range(k):
        full[:, j:j + (T - 1) * stride + 1:stride] += x.double() @ w[:, :, j].double()
    return full[:, pad:pad + T * stride] + b.double()


def resblock_step(x, w1, b1, w2, b2, dilation, slope, padded=None):
    """One ResBlock1 step, ``x + conv2(lrelu(conv1_dilated(lrelu(x))))``.  ``padded``: a function ``[B, T, C] -> [B, T + 2 halo, C]``
    that pads a convolution's input (reflect mode); None = zeros."""
    pd = (lambda v: None) if padded is None else padded
    a = lrelu(x, slope)
    t = lrelu(conv1d_same(a, w1, b1, dilation, pd(a)), slope)
    return x.double() + conv1d_same(t, w2, b2, 1, pd(t))


def mrf_mix(a, b, c, slope):
    """LeakyReLU of the mean of the three ResBlock outputs (the activation belongs to the layer that follows)."""
    return lrelu((a.double() + b.double() + c.double()) / 3.0, slope)


def conv_post(x_padded, w, b, k):
    """Conv1d(C -> 1, k) + tanh on ``x_padded [B, T + k - 1, C]`` (the input with its (k - 1) / 2 rows of padding on either side, whatever
    they hold); ``w [1, C, k]``, ``b`` a number.  Returns ``(tanh(y) [B, T], mass [B, T])`` with ``mass = sum |w| |x| + |b|``, the
    magnitude that the rounding errors of an accumulation of y scale with."""
    assert tuple(w.shape) == (1, x_padded.shape[2], k) and k % 2 == 1
    T = x_padded.shape[1] - (k - 1)
    xp, w = x_padded.double(), w.double()
    y = torch.full((xp.shape[0], T), float(b), dtype=torch.float64)
    mass = torch.full_like(y, abs(float(b)))
    for j in range(k):
        y += xp[:, j:j + T] @ w[0, :, j]
        mass += xp[:, j:j + T].abs() @ w[0, :, j].abs()
    return torch.tanh(y), mass


def halo_fill(map_, T, halo, mode):
    """``map_ [B, T + 2 * halo, C]`` with its halo rows rewritten: mode 0 zeros; mode 1 the reflection about the first / last sample
    (``x[-j] = x[j]``, ``x[T-1+j] = x[T-1-j]``, torch's "reflect") for j = 1 .. min(halo, T - 1), zeros beyond.  Keeps the dtype."""
    assert map_.shape[1] == T + 2 * halo and mode in (0, 1)
    out = map_.clone()
    out[:, :halo] = 0
    out[:, halo + T:] = 0
    if mode == 1:
        for j in range(1, min(halo, T - 1) + 1):
            out[:, halo - j] = map_[:, halo + j]
            out[:, halo + T - 1 + j] = map_[:, halo + T - 1 - j]
    return out


def pack_mel(mel, pad):
    """``mel [B, C, T]`` (torch layout) -> channels-last ``[B, T + 2 * pad, C]``, the first / last frame replicated ``pad`` times
    (``F.pad(mel, (pad, pad), "replicate")``).  Keeps the dtype."""
    T = mel.shape[2]
    idx = (torch.arange(T + 2 * pad) - pad).clamp(0, T - 1)
    return mel[:, :, idx].transpose(1, 2).contiguous()


def generator(mel, sd, cfg, padding_mode="zeros", inference_padding=0):
    """``mel [B, n_mels, T] -> wav [B, 1, (T + 2 * inference_padding) * hop]`` in float64, composed from the helpers above."""
    assert padding_mode in ("zeros", "reflect") and len(cfg.resblock_kernel_sizes) == 3
    ks, ds, slope = cfg.resblock_kernel_sizes, cfg.resblock_dilations, cfg.leaky_slope
    halo = max((max(ks) - 1) * max(ds) // 2, (cfg.pre_kernel - 1) // 2, (cfg.post_kernel - 1) // 2)
    mode = int(padding_mode == "reflect")

    def padded(v):
        m = torch.zeros(v.shape[0], v.shape[1] + 2 * halo, v.shape[2], dtype=torch.float64)
        m[:, halo:halo + v.shape[1]] = v
        return halo_fill(m, v.shape[1], halo, mode)

    x = pack_mel(mel.double(), inference_padding)
    x = lrelu(conv1d_same(x, sd["conv_pre.weight"], sd["conv_pre.bias"], 1, padded(x)), slope)
    nstage = len(cfg.upsample_rates)
    for i, r in enumerate(cfg.upsample_rates):
        x = conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], r)
        outs = []
        for j in range(3):
            y = x
            for d, dil in enumerate(ds):
                w1, b1, w2, b2 = (sd[f"resblocks.{i * 3 + j}.convs{c}.{d}.{n}"] for c in (1, 2) for n in ("weight", "bias"))
                y = resblock_step(y, w1, b1, w2, b2, dil, slope, padded)
            outs.append(y)
        x = mrf_mix(*outs, slope if i < nstage - 1 else 0.01)            # F.leaky_relu's default before conv_post
    k = cfg.post_kernel
    xp = padded(x)[:, halo - (k - 1) // 2:halo + x.shape[1] + (k - 1) // 2]
    wav, _ = conv_post(xp, sd["conv_post.weight"], float(sd["conv_post.bias"][0]), k)
    return wav[:, None]
