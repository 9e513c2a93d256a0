"""``captum.influence``-compatible front end (SimilarityInfluence, TracInCPFast) over ``addvisor_hip.influence``, mapped the way
``captum.concept`` maps onto ``HipTCAV``: ``model`` is a ``captum_saliency.Wav2vec2LogReg`` (anything exposing
``.hip_attribution()``), a layer is ``"hidden_states.<l>"`` or the integer ``l``, and there is no autograd fallback.

Differences from Captum 0.7:

- a dataset is a ``[N, L]`` waveform tensor or an iterable of ``[n, L]`` batches (TracInCPFast: ``(waves, labels)`` or an
  iterable of such pairs), not a ``torch.utils.data.Dataset``; it is embedded ONCE, at construction, and kept on the device --
  ``activation_dir`` / ``load_src_from_disk`` do not exist (``HipInfluenceIndex.save`` / ``load`` write one ``.npz``);
- ``similarity_metric`` is one of the two functions of this module (they name the metric; the arithmetic is a HIP kernel);
- ``TracInCPFast``: a checkpoint is ``(coef [H], intercept, lr)``, so there is no ``checkpoints_load_func``; the loss is the
  classifier's own BCE-with-logits per sample, so ``loss_fn`` must be None; ``final_fc_layer`` is the model's logistic
  regression whatever is passed.  The embedder is frozen: one forward per clip serves every checkpoint;
- ``influence`` takes ``k`` up to 256; ``unpack_inputs`` / ``show_progress`` are not supported.
- ``HipLogisticInfluence`` (influence functions, Koh & Liang 2017) has no Captum 0.7 counterpart and is re-exported as it is.

Parity with Captum is unpinned (captum is absent): the restatement is from its source and the papers."""
import torch

from addvisor_hip.influence import HipInfluenceIndex, HipLogisticInfluence, HipSimilarityInfluence, HipTracInCPFast
from captum.concept import _layer_index

__all__ = ["SimilarityInfluence", "TracInCPFast", "cosine_similarity", "euclidean_distance", "HipLogisticInfluence", "HipInfluenceIndex"]


def cosine_similarity(test, train, replace_nan=0):
    """Names the cosine metric of ``SimilarityInfluence`` (``advh_influence_cosine``: a zero row gives 0)."""
    raise NotImplementedError("cosine_similarity names a metric of SimilarityInfluence (HIP build); it is not called on tensors")


def euclidean_distance(test, train):
    """Names the euclidean metric of ``SimilarityInfluence`` (``advh_influence_sqdist`` and a square root)."""
    raise NotImplementedError("euclidean_distance names a metric of SimilarityInfluence (HIP build); it is not called on tensors")


def _engine(model, what: str):
    if hasattr(model, "hip_mask_attribution") or not hasattr(model, "hip_attribution"):
        raise TypeError(f"captum.influence.{what} (HIP build) only explains captum_saliency.Wav2vec2LogReg models")
    return model.hip_attribution()


def _batches(data):
    return [data] if torch.is_tensor(data) or (isinstance(data, tuple) and len(data) == 2 and torch.is_tensor(data[0])) else data


class SimilarityInfluence:
    def __init__(self, module, layers, influence_src_dataset, activation_dir=None, model_id="", similarity_metric=cosine_similarity,
                 similarity_direction="max", batch_size=16, pool="none", memory_budget=8 << 30, **kwargs):
        att = _engine(module, "SimilarityInfluence")
        if activation_dir is not None:
            raise NotImplementedError("the activations stay on the device; activation_dir must be None (HipInfluenceIndex.save writes a file)")
        if kwargs:
            raise NotImplementedError(f"unsupported arguments: {sorted(kwargs)}")
        if similarity_metric not in (cosine_similarity, euclidean_distance):
            raise NotImplementedError("similarity_metric must be captum.influence.cosine_similarity or euclidean_distance: "
                                      "a Python callable cannot run on the HIP path")
        self.layers = [layers] if isinstance(layers, (str, int)) else list(layers)
        self._index_of = {name: _layer_index(name) for name in self.layers}
        self.index = HipInfluenceIndex(att, list(self._index_of.values()), pool=pool, internal_batch_size=batch_size, memory_budget=memory_budget)
        for waves in _batches(influence_src_dataset):
            self.index.add(waves)
        metric = "cosine" if similarity_metric is cosine_similarity else "euclidean"
        self._engines = {name: HipSimilarityInfluence(self.index, l, metric, similarity_direction) for name, l in self._index_of.items()}

    def influence(self, inputs, top_k=1, additional_forward_args=None, load_src_from_disk=True, **kwargs):
        """``{layer: (indices [B, k], scores [B, k])}``, Captum's result."""
        if additional_forward_args is not None:
            raise NotImplementedError("the classifier takes the waveform alone; additional_forward_args must be None")
        if kwargs:
            raise NotImplementedError(f"unsupported arguments: {sorted(kwargs)}")
        return {name: eng.influence(inputs, top_k=top_k) for name, eng in self._engines.items()}


class TracInCPFast:
    def __init__(self, model, final_fc_layer, train_dataset, checkpoints, checkpoints_load_func=None, loss_fn=None, batch_size=16,
                 test_loss_fn=None, vectorize=False, memory_budget=8 << 30):
        att = _engine(model, "TracInCPFast")
        if checkpoints_load_func is not None:
            raise NotImplementedError("a checkpoint is (coef, intercept, lr): checkpoints_load_func must be None")
        if loss_fn is not None or test_loss_fn is not None:
            raise NotImplementedError("the loss is the classifier's own BCE-with-logits per sample: loss_fn and test_loss_fn must be None")
        self.index = HipInfluenceIndex(att, (), internal_batch_size=batch_size, memory_budget=memory_budget)
        for batch in _batches(train_dataset):
            if not (isinstance(batch, (tuple, list)) and len(batch) == 2):
                raise ValueError("train_dataset must be (waves [N, L], labels [N]) or an iterable of such pairs")
            self.index.add(batch[0], batch[1])
        self._engine = HipTracInCPFast(self.index, checkpoints)

    def influence(self, inputs, k=None, proponents=True, unpack_inputs=True, show_progress=False):
        """``inputs``: ``(waves [B, L], labels [B])``.  ``k=None``: the ``[B, N]`` scores; otherwise ``(indices, scores)``."""
        if show_progress:
            raise NotImplementedError("show_progress is not supported")
        if not (isinstance(inputs, (tuple, list)) and len(inputs) == 2):
            raise ValueError("inputs must be (waves [B, L], labels [B])")
        return self._engine.influence(inputs[0], inputs[1], k=k, proponents=proponents)

    def self_influence(self, inputs=None, show_progress=False):
        if inputs is not None:
            raise NotImplementedError("self_influence is computed over the training set given at construction; inputs must be None")
        return self._engine.self_influence()
