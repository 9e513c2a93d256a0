"""Reference driver of the ragged-batch tests: the per-clip-alone oracle and the table of clip lengths.

One definition: for a batch ``wave [B, L]`` with ``lengths[b]`` valid samples in clip b, the result for clip b is what the model
gives for ``wave[b, :lengths[b]]`` run ALONE, unpadded -- ``oracle/wav2vec2_ref.hidden_states`` / ``classify`` called once per
clip on the cropped clip.  Kept free of GPU imports: tests/test_ragged_ref_cpu.py holds it against HF's ``attention_mask``.
"""
import functools

import torch

from addvisor_hip import synthetic as syn
from oracle import wav2vec2_ref

L = 4000                                     # the batch length of the table: T = 12 frames
# (samples, frames, the claim the length stands for)
TABLE = (
    (4000, 12, "full length"),
    (3999, 12, "one sample short, same T"),
    (2500, 7, "T = 7"),
    (1040, 3, "T = 3"),
    (720, 2, "T = 2"),
    (719, 1, "T = 1, one sample under two frames"),
    (400, 1, "T = 1, shortest"),
)
LENGTHS = tuple(n for n, _, _ in TABLE)


def frames(cfg, n):
    """Valid encoder frames of a clip of ``n`` samples: the feature encoder's output-length formula, layer by layer."""
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1
    return n


def receptive_end(cfg, t):
    """One past the last sample that frame ``t`` of the last feature-encoder layer reads."""
    last = t                                 # index of the last row read, walked down the layers
    for k, s in zip(reversed(cfg.conv_kernel), reversed(cfg.conv_stride)):
        last = last * s + k - 1
    return last + 1


def min_length(cfg):
    return receptive_end(cfg, 0)


@functools.lru_cache(maxsize=None)
def clips(B, n, seed):
    """``B`` clips of ``n`` samples (the project's synthetic speech-like clips).  Shared: never modify."""
    return syn.make_clips(B, n, seed=seed)


def layer_of(cfg):
    return min(cfg.layer_index, cfg.num_hidden_layers)


def per_clip_hidden(wave, lengths, sd, cfg, normalize=True, layers=None):
    """[hidden_states of clip b run alone, cropped to lengths[b]] -- each ``[T_b, H]`` (``layers`` None: the embedder's
    layer) or a list of them for the indices in ``layers``.  ``normalize`` off: the clip is taken as already normalised."""
    out = []
    for b, n in enumerate(lengths):
        x = wave[b:b + 1, :n]
        x = wav2vec2_ref.zero_mean_unit_var_norm(x) if normalize else x
        hs = wav2vec2_ref.hidden_states(x, sd, cfg, upto=cfg.layer_index if layers is None else max(layers))
        out.append(hs[layer_of(cfg)][0] if layers is None else [hs[i][0] for i in layers])
    return out


def per_clip_classify(hidden, coef, icpt):
    """(logits [B, 1], probs [B, 1]) from the per-clip hidden states: each clip pools over its own frames."""
    pooled = torch.stack([h.mean(0) for h in hidden])
    return wav2vec2_ref.logreg(pooled, coef, icpt)
