"""CPU-only: the reference the long-clip GPU tests lean on.  The committed goldens stop at 5 s, so ``oracle/wav2vec2_ref`` at
T = 299 (6 s) and T = 513 frames is held here against ``transformers``' ``Wav2Vec2Model`` with the same weights: both in float64
(the restatement is the same function: 1e-10 of max|ref|; measured 3e-15), and the oracle in float32 -- what the GPU tests compare
with -- against the float64 model (bound 5e-6 of max|ref|, the bound of tests/test_ragged_ref_cpu.py; measured 1e-6)."""
import pytest
import torch

import ragged_ref as RR
from addvisor_hip import synthetic as syn
from oracle import wav2vec2_ref

transformers = pytest.importorskip("transformers")
torch.set_grad_enabled(False)

TOL_F64, TOL_F32 = 1e-10, 5e-6
LAYERS = (0, 5, 9)
LENGTHS = {96000: 299, 164240: 513}
CONFIGS = {"tiny_group": lambda: syn.tiny_config(False), "tiny_layer": lambda: syn.tiny_config(True),
           "head120": lambda: syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480)}


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_is_hf_beyond_256_frames(name, L):
    cfg = CONFIGS[name]()
    sd = syn.embedder_weights(cfg)
    m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**cfg.hf_kwargs()))
    m.load_state_dict(sd, strict=True)
    m = m.eval().double()
    x = wav2vec2_ref.zero_mean_unit_var_norm(RR.clips(1, L, 91))
    hf = m(x.double(), output_hidden_states=True).hidden_states
    assert hf[0].shape[1] == LENGTHS[L] == RR.frames(cfg, L)
    sd64 = {k: v.double() for k, v in sd.items()}
    ref64 = wav2vec2_ref.hidden_states(x.double(), sd64, cfg, upto=max(LAYERS))
    ref32 = wav2vec2_ref.hidden_states(x, sd, cfg, upto=max(LAYERS))
    for l in LAYERS:
        top = hf[l].abs().max()
        e64 = ((ref64[l] - hf[l]).abs().max() / top).item()
        e32 = ((ref32[l].double() - hf[l]).abs().max() / top).item()
        print(f"{name} T={LENGTHS[L]} hidden_states[{l}]: oracle fp64 vs HF fp64 {e64:.1e}, oracle fp32 vs HF fp64 {e32:.1e}")
        assert e64 <= TOL_F64 and e32 <= TOL_F32, (name, L, l, e64, e32)
