"""CPU-only: the definition the ragged-batch tests hold the kernels to (tests/ragged_ref.py) is HF's ``attention_mask``
semantics for layer-norm feature encoders, and deliberately not HF's for group-norm ones.

HF steps with a mask (modeling_wav2vec2.py): the feature extractor normalises over the valid samples (done here by hand, as
HF's Wav2Vec2FeatureExtractor does), ``_get_feature_vector_attention_mask`` turns sample counts into frame counts,
``hidden_states[~expand_attention_mask] = 0`` after the projection, and the additive -inf mask on padded keys.  HF's padded rows
are not compared.  Measured: 1.0e-6 of max|ref| on the valid frames at hidden states 0, 5 and 9 (bound 5e-6: the margin covers
thread-count and BLAS differences).  For ``feat_extract_norm="group"`` HF lets the padding into GroupNorm's statistics (its
model card says not to pass a mask); measured 6.8e-4 (one padded sample) .. 0.97 (400 of 4000 samples) of max|ref|, above the
GPU tolerance of 1e-4, so the per-clip-alone definition is a choice and this test documents it."""
import pytest
import torch

import ragged_ref as RR
from addvisor_hip import synthetic as syn
from oracle import wav2vec2_ref

transformers = pytest.importorskip("transformers")
torch.set_grad_enabled(False)

TOL_HF = 5e-6
LAYERS = (0, 5, 9)
GPU_TOL_HID = 1e-4                           # tests/test_gpu_split.py TOL_HID


def build_hf(cfg):
    m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**cfg.hf_kwargs()))
    m.load_state_dict(syn.embedder_weights(cfg), strict=True)
    return m.eval()


def masked_batch(lengths):
    """(input_values [B, L] normalised over the valid part with zeros behind, mask [B, L])."""
    wave = RR.clips(len(lengths), RR.L, 91)
    x = torch.zeros_like(wave)
    mask = torch.zeros(wave.shape, dtype=torch.long)
    for b, n in enumerate(lengths):
        x[b, :n] = wav2vec2_ref.zero_mean_unit_var_norm(wave[b:b + 1, :n])[0]
        mask[b, :n] = 1
    return wave, x, mask


def hf_vs_alone(cfg):
    """Worst |HF masked - clip alone| / max|ref| over the valid frames, per clip and layer."""
    sd = syn.embedder_weights(cfg)
    wave, x, mask = masked_batch(RR.LENGTHS)
    hs = build_hf(cfg)(x, attention_mask=mask, output_hidden_states=True).hidden_states
    ref = RR.per_clip_hidden(wave, RR.LENGTHS, sd, cfg, layers=LAYERS)
    out = {}
    for b, n in enumerate(RR.LENGTHS):
        Tb = RR.frames(cfg, n)
        for i, l in enumerate(LAYERS):
            r = ref[b][i]
            assert r.shape[0] == Tb
            out[(n, l)] = ((hs[l][b, :Tb] - r).abs().max() / r.abs().max()).item()
    return out


def test_per_clip_alone_is_hf_attention_mask_for_layer_norm_encoders():
    err = hf_vs_alone(syn.tiny_config(stable=True))
    print("HF attention_mask vs clip alone (layer norm):", {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) <= TOL_HF, err


def test_group_norm_encoders_differ_from_hf_by_design():
    err = hf_vs_alone(syn.tiny_config(stable=False))
    print("HF attention_mask vs clip alone (group norm):", {k: f"{v:.1e}" for k, v in err.items()})
    short = [v for (n, _), v in err.items() if n < RR.L]
    assert min(short) > GPU_TOL_HID, err                 # every padded clip, the one-sample one included (6.8e-4): HF's GroupNorm saw the padding
    full = [v for (n, _), v in err.items() if n == RR.L]
    assert max(full) <= TOL_HF, err                      # nothing to pad: the two agree


def test_frame_lengths_match_hf():
    cfg = syn.tiny_config(stable=True)
    m = build_hf(cfg)
    ns = list(RR.LENGTHS) + [401, 639, 640, 16000, 12345, 64000]
    hf = m._get_feat_extract_output_lengths(torch.tensor(ns)).tolist()
    assert hf == [RR.frames(cfg, n) for n in ns]
    from addvisor_hip.embedder import HipEmbedder        # the host's own formula, without constructing an embedder
    emb = HipEmbedder.__new__(HipEmbedder)
    emb.cfg = cfg
    assert emb.frame_lengths(ns) == hf and emb.frame_lengths(torch.tensor(ns)) == hf
    assert emb.min_length() == RR.min_length(cfg) == 400


def test_last_valid_frame_reads_valid_samples_only():
    cfg = syn.tiny_config(stable=True)
    for n, T, _ in RR.TABLE:
        assert RR.receptive_end(cfg, T - 1) <= n < RR.receptive_end(cfg, T), (n, T)   # frame T - 1 fits, frame T does not


def test_every_claim_of_the_length_table():
    cfg = syn.tiny_config(stable=True)
    by_n = {n: T for n, T, _ in RR.TABLE}
    assert all(RR.frames(cfg, n) == T for n, T, _ in RR.TABLE)
    assert RR.frames(cfg, RR.L) == 12 and by_n[4000] == 12                      # full length
    assert by_n[3999] == by_n[4000]                                             # one sample short, same T
    assert (by_n[2500], by_n[1040], by_n[720]) == (7, 3, 2)
    assert by_n[719] == 1 and RR.frames(cfg, 720) == 2                          # one sample under two frames
    assert by_n[400] == 1 and RR.frames(cfg, 399) == 0 and RR.min_length(cfg) == 400   # shortest
    assert max(RR.LENGTHS) == RR.L and len(set(RR.LENGTHS)) == len(RR.LENGTHS)
    assert syn.tiny_config(stable=False).conv_kernel == cfg.conv_kernel         # one table for both configs
