"""Reference of the ragged gradient chain: float64 autograd of the oracle on each cropped clip ALONE, zero-filled to ``L``.

One definition (tests/ragged_ref.py): everything the chain returns for clip b of ``wave [B, L]`` with ``lengths[b]`` valid
samples is what the model gives for ``wave[b, :lengths[b]]`` run alone, unpadded.  ``ragged_ref.per_clip_hidden`` builds the
per-clip graphs from one float64 leaf ``wave``, so autograd's gradient at the leaf is already the per-clip gradient in
``[:lengths[b]]`` and exactly 0 behind; the chain below the encoder goes through ``fe_backward_ref.lower_chain_vjp`` per clip.
Kept free of GPU imports: tests/test_ragged_grad_ref_cpu.py pins it against finite differences and HF's ``attention_mask``.
"""
import functools

import torch

import fe_backward_ref as FE
import ragged_ref as RR
from addvisor_hip import synthetic as syn

F64 = torch.float64


def to64(sd):
    return {k: v.detach().to(F64) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def model(name):
    """(cfg, state dict, coef, intercept) of a test model.  Shared: never modify."""
    cfg = {"tiny_layer": lambda: syn.tiny_config(True), "tiny_group": lambda: syn.tiny_config(False),
           "tiny_layer_depth9": lambda: syn.tiny_config(True, num_hidden_layers=9), "base": syn.base_config,
           "xlsr": lambda: syn.xlsr2b_config(num_hidden_layers=2, layer_index=2)}[name]()
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    return cfg, syn.embedder_weights(cfg), coef, icpt


def logits_of(hidden, coef, icpt):
    """fp64 logits [B] of per-clip hidden states: each clip pools over its own frames."""
    c = torch.as_tensor(coef, dtype=F64).reshape(-1)
    return torch.stack([(h.mean(0) * c).sum() + float(torch.as_tensor(icpt).reshape(-1)[0]) for h in hidden])


def graph(wave, lengths, mdl, layers):
    """(leaf wave [B, L] fp64, [[hidden_states[l] of clip b alone for l in layers] for b]) with the autograd graph attached."""
    cfg, sd = mdl[0], mdl[1]
    x = wave.detach().to(F64).requires_grad_(True)
    with torch.enable_grad():
        hs = RR.per_clip_hidden(x, lengths, to64(sd), cfg, layers=list(layers))
    return x, hs


def logit(wave, lengths, mdl):
    """fp64 logits [B], no graph."""
    cfg, _, coef, icpt = mdl
    _, hs = graph(wave, lengths, mdl, [RR.layer_of(cfg)])
    return logits_of([h[0] for h in hs], coef, icpt).detach()


def input_gradient(wave, lengths, mdl, seed=None):
    """(d (seed . logit) / d wave [B, L] fp64 -- clip b's gradient in ``[:lengths[b]]``, 0 behind --, logits [B] fp64);
    ``seed [B]``: dL / d logit per clip (None: ones)."""
    cfg, _, coef, icpt = mdl
    x, hs = graph(wave, lengths, mdl, [RR.layer_of(cfg)])
    with torch.enable_grad():
        lg = logits_of([h[0] for h in hs], coef, icpt)
        s = torch.ones_like(lg) if seed is None else seed.detach().to(F64).reshape(-1)
        (dx,) = torch.autograd.grad((lg * s).sum(), x)
    return dx.detach(), lg.detach()


def layer_gradient(wave, lengths, mdl, layer):
    """[d logit / d hidden_states[layer] of clip b alone, ``[T_b, H]`` fp64]."""
    from oracle import wav2vec2_ref
    cfg, sd, coef, icpt = mdl
    sdd, out = to64(sd), []
    for b, n in enumerate(lengths):                          # per_clip_hidden hands out views: the graph runs through the whole tensors
        with torch.enable_grad():
            x = wav2vec2_ref.zero_mean_unit_var_norm(wave[b:b + 1, :n].detach().to(F64)).requires_grad_(True)
            hs = wav2vec2_ref.hidden_states(x, sdd, cfg, upto=cfg.layer_index)
            lg = logits_of([hs[RR.layer_of(cfg)][0]], coef, icpt)
            (g,) = torch.autograd.grad(lg.sum(), hs[layer])
        out.append(g[0].detach())
    return out


def lower_vjp(wave, lengths, mdl, S):
    """``d sum(hidden_states[0] * S[b, :T_b]) / d wave`` per clip alone, zero-filled: ``[B, L]`` fp64.  ``S [B, T, H]``."""
    cfg, sd = mdl[0], mdl[1]
    out = torch.zeros(wave.shape, dtype=F64)
    for b, n in enumerate(lengths):
        Tb = RR.frames(cfg, n)
        _, dx = FE.lower_chain_vjp(cfg, sd, wave[b:b + 1, :n], S[b:b + 1, :Tb])
        out[b, :n] = dx[0]
    return out


def padded_input_gradient(wave, lengths, mdl):
    """The mistake: the padded batch differentiated as ONE batch of full-length clips (zeros behind each length), fp64."""
    w = wave.clone()
    for b, n in enumerate(lengths):
        w[b, n:] = 0.0
    return input_gradient(w, [wave.shape[1]] * wave.shape[0], mdl)[0]


def clip_errors(got, ref, lengths):
    """Per clip over ``[:lengths[b]]``: (max |got - ref| / max |ref|, cosine)."""
    out = []
    for b, n in enumerate(lengths):
        g, r = got[b, :n].to(F64), ref[b, :n].to(F64)
        out.append((((g - r).abs().max() / r.abs().max()).item(), torch.nn.functional.cosine_similarity(g, r, dim=0).item()))
    return out
