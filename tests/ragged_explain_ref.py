"""Reference driver of the ragged explanation tests: the per-clip-alone oracle and the shared table of clip lengths.

One definition: clip b of a ragged batch ``wave [B, L]`` with ``lengths[b] = n_b`` valid samples gets what the explanation
pipeline gives for ``wave[b, :n_b]`` run ALONE at an audio length of exactly ``n_b`` samples -- ``torch.stft`` reflecting at
``n_b``, the U-Net on the ``512 x W_b`` crop, the mask embedded with zeros outside the crop, ``torch.istft(length=n_b)`` of both
branches, the classifier pooling over each waveform's own frames.  Built from ``oracle.signal_ref`` / ``unet_ref`` /
``wav2vec2_ref`` with ``audio_length=n_b, sr=1``: the sample count goes in as it is, never as seconds
(``int(n / 16000 * 16000)`` can round down).  In the batch's buffers everything past a clip's extent is exactly 0.
Kept free of GPU imports; tests/test_ragged_explain_ref_cpu.py asserts the table's claims."""
import functools

import torch

from addvisor_hip import synthetic as syn
from oracle import signal_ref as S, unet_ref as U, wav2vec2_ref as W

L, HOP, WIN, H = 8000, 322, 644, 512             # the buffer: T = 25 frames, W = 24 mask columns
# (samples, T_b, W_b, what the length stands for)
TABLE = (
    (8000, 25, 24, "full"),
    (7999, 25, 24, "one sample short, same T"),
    (7728, 25, 24, "24 hops: the first length with 25 frames"),
    (7727, 24, 24, "the last with 24"),
    (6440, 21, 20, ""),
    (5151, 16, 16, ""),
    (2576, 9, 8, ""),
    (1288, 5, 4, ""),
    (966, 4, 4, "shortest"),
)
LENGTHS = tuple(n for n, _, _, _ in TABLE)
TOO_SHORT = 965                                  # T_b = 3: no mask column
# bars of tests/test_gpu_pipeline.py
TOL = {"f32": dict(prob=1e-4, mask=2e-5, wave=5e-5), "f16": dict(prob=1e-2, mask=1.5e-2, wave=2e-2)}
PROBS = ("predictions", "theta_out", "masked_predictions")


def frame_counts(n, hop=HOP):
    T = 1 + n // hop
    return T, 4 * (T // 4)


@functools.lru_cache(maxsize=None)
def models():
    """(cfg, embedder weights, U-Net weights, coef, intercept) of the tests: the tiny embedder, the default synthetic U-Net."""
    cfg = syn.tiny_config(False)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    return cfg, syn.embedder_weights(cfg), syn.unet_weights(), coef, icpt


@functools.lru_cache(maxsize=None)
def clips(B=len(TABLE), n=L, seed=3):
    """The table's clips, one per length.  Shared: never modify."""
    return syn.make_clips(B, n, seed=seed)


def explain_alone(w, domain="log1p", hop=HOP, win=WIN, weights=None):
    """The oracle on ONE clip ``w [n]`` at an audio length of exactly ``n`` samples (``weights``: another tuple like ``models()``)."""
    cfg, emb_sd, unet_sd, coef, icpt = weights or models()
    n = w.numel()
    T, Wb = frame_counts(n, hop)
    if Wb < 4:
        raise ValueError(f"a clip of {n} samples has {T} frames: no mask column")
    w = w[None]
    X, mag, phase = S.compute_stft(w, hop=hop, win=win, audio_length=n, sr=1)
    assert X.shape == (1, 513, T)
    _, p_clean = W.classify(w, emb_sd, cfg, coef, icpt)
    mask = U.unet_forward(U.crop_for_unet(mag), unet_sd)[:, 0]
    assert mask.shape == (1, H, Wb)
    rel, irr = S.apply_mask(S.embed_mask(mask, 513, T), mag, phase, domain)
    w_in = S.compute_invert_stft(rel, hop=hop, win=win, audio_length=n, sr=1)
    w_out = S.compute_invert_stft(irr, hop=hop, win=win, audio_length=n, sr=1)
    _, p_in = W.classify(w_in, emb_sd, cfg, coef, icpt)
    _, p_out = W.classify(w_out, emb_sd, cfg, coef, icpt)
    return dict(spec=X[0], mag=mag[0], mask=mask[0], wave_in=w_in[0], wave_out=w_out[0], predictions=p_clean[0],
                theta_out=p_in[0], masked_predictions=p_out[0])


def assemble(per_clip, Lbuf, hop=HOP):
    """The per-clip results in the batch's buffers, zeros past every clip's extent."""
    B, (T, Wd) = len(per_clip), frame_counts(Lbuf, hop)
    out = dict(spec=torch.zeros(B, 513, T, dtype=torch.complex64), mag=torch.zeros(B, 513, T), mask=torch.zeros(B, H, Wd),
               wave_in=torch.zeros(B, Lbuf), wave_out=torch.zeros(B, Lbuf))
    for b, r in enumerate(per_clip):
        for k in ("spec", "mag", "mask"):
            out[k][b, :r[k].shape[0], :r[k].shape[1]] = r[k]
        for k in ("wave_in", "wave_out"):
            out[k][b, :r[k].numel()] = r[k]
    for k in PROBS:
        out[k] = torch.stack([r[k] for r in per_clip])
    return out


def explain_ragged(waves, lengths, domain="log1p", Lbuf=None, weights=None):
    """The definition on a batch: every clip alone, assembled."""
    return assemble([explain_alone(waves[b, :n], domain, weights=weights) for b, n in enumerate(lengths)],
                    waves.shape[1] if Lbuf is None else Lbuf)


LONG_L, LONG_LENGTHS = 83200, (83200, 40000, 966)    # 259 spectrogram and encoder frames: past the whole-clip attention's 256


@functools.lru_cache(maxsize=None)
def long_reference(domain="log1p"):
    """A batch beyond 256 frames next to the shortest clip, each alone.  Shared: never modify."""
    with torch.no_grad():
        w = syn.make_clips(len(LONG_LENGTHS), LONG_L, seed=4)
        return w, explain_ragged(w, LONG_LENGTHS, domain)


@functools.lru_cache(maxsize=None)
def table_reference(domain="log1p"):
    """The table's nine clips, each alone, in an ``L``-sample buffer.  Computed once per domain; shared: never modify."""
    with torch.no_grad():
        return explain_ragged(clips(), LENGTHS, domain)


def padded_mask(w, n):
    """The padded-batch mistake: the mask of ``w[:n]`` zero-padded to the buffer's ``L`` samples, on the clip's own columns."""
    _, _, unet_sd, _, _ = models()
    x = torch.zeros(1, L)
    x[0, :n] = w[:n]
    _, mag, _ = S.compute_stft(x, hop=HOP, win=WIN, audio_length=L, sr=1)
    return U.unet_forward(U.crop_for_unet(mag), unet_sd)[0, 0, :, :frame_counts(n)[1]]
