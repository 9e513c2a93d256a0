"""Drop-in for the reference's ``classifier_embedder`` module (classifier_embedder.py:1-63):
same names (``classifier``, ``processor``, ``wav2vec2``, ``TorchLogReg``, ``zero_mean_unit_var_norm``),
MI355X kernels underneath, and NO import-time fetch: see ``addvisor_hip.runtime`` for where weights
come from."""
import torch
import torch.nn as nn

from addvisor_hip import runtime as _rt


class _Lazy:
    def __init__(self, factory):
        object.__setattr__(self, "_f", factory)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_f")(), name)


classifier = _Lazy(_rt.classifier)          # .coef_ (1,H), .intercept_ (1,)   (classifier_embedder.py:12)
processor = None                            # the HF feature extractor is never used by the hot path (:13)


class _HiddenStates:
    """``output.hidden_states``: index k runs the first k encoder layers on the GPU."""

    def __init__(self, x, lengths=None):
        self._x = x
        self._lengths = lengths

    def __getitem__(self, k):
        emb = _rt.hip_embedder()
        if k != emb.cfg.layer_index:
            raise IndexError(f"this embedder is built for hidden_states[{emb.cfg.layer_index}] "
                             "(set ADDVISOR_LAYER_INDEX to change it)")
        hid, _, _ = emb.forward(self._x, normalize=False, lengths=self._lengths)
        return hid


class _Output:
    def __init__(self, x, lengths=None):
        self.hidden_states = _HiddenStates(x, lengths)


def mask_lengths(attention_mask, shape):
    """Per-clip lengths of a 0/1 right-padded ``attention_mask`` of ``shape`` ``[B, L]``; a mask of another shape, with other
    values or with holes (a 1 behind a 0) raises ``ValueError``."""
    m = torch.as_tensor(attention_mask)
    if m.dim() == 1:
        m = m[None]
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"attention_mask has shape {tuple(m.shape)}, input_values {tuple(shape)}")
    m = m.cpu()
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("attention_mask must hold 0 and 1 only")
    m = m.to(torch.int64)
    lengths = m.sum(-1)
    if not torch.equal(m, (torch.arange(m.shape[1])[None] < lengths[:, None]).to(torch.int64)):
        raise ValueError("attention_mask must be right-padded: ones up to each clip's length, zeros behind (a mask with holes "
                         "is not supported)")
    return lengths.tolist()


class _Wav2Vec2:
    """``wav2vec2(input_values, output_hidden_states=True).hidden_states[9]`` (audioprocessor.py:76-77).
    ``input_values`` is the already normalised waveform, as in the reference.  ``attention_mask`` (HF's argument: 0/1,
    right-padded) makes the batch ragged: clip ``b`` is its first ``mask[b].sum()`` samples, expected normalised over that valid
    part as HF's feature extractor delivers it; samples behind read as 0 and rows past the clip's frames come back as zeros.
    For group-norm feature encoders the result is that of the clip run alone, which HF's masked call is not (HF lets the padding
    into GroupNorm's statistics)."""

    def __call__(self, input_values, attention_mask=None, output_hidden_states=True):
        x = input_values
        if x.dim() == 1:
            x = x[None]
        lengths = None if attention_mask is None else mask_lengths(attention_mask, x.shape)
        return _Output(x.to(_rt.device(), torch.float32).contiguous(), lengths)

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    @property
    def config(self):
        return _rt.embedder_config_and_weights()[0]


wav2vec2 = _Wav2Vec2()


class TorchLogReg(nn.Module):
    """classifier_embedder.py:21-38: Linear(H, 1) initialised from the sklearn model; (logits, probs)."""

    def __init__(self):
        super().__init__()
        clf = _rt.classifier()
        self.linear = nn.Linear(clf.coef_.shape[1], 1)
        self.linear.weight = nn.Parameter(torch.tensor(clf.coef_, dtype=torch.float32), requires_grad=False)
        self.linear.bias = nn.Parameter(torch.tensor(clf.intercept_, dtype=torch.float32), requires_grad=False)

    def forward(self, x):
        logits = self.linear(x)
        return logits, torch.sigmoid(logits)


def zero_mean_unit_var_norm(input_values):
    """classifier_embedder.py:59-63 (kept as tensor ops so autograd callers keep working; the fused HIP
    front end applies the same normalisation inside ``AudioProcessor.extract_features``)."""
    mean = input_values.mean(dim=-1, keepdim=True)
    std = input_values.std(dim=-1, keepdim=True)
    return (input_values - mean) / (std + 1e-7)
