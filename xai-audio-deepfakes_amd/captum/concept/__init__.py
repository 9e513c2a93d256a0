"""``captum.concept``-compatible front end (TCAV, Kim et al. 2018) over ``addvisor_hip.concept.HipTCAV``, mapped the way
``captum.attr`` maps onto ``HipAttribution``: ``model`` is a ``captum_saliency.Wav2vec2LogReg`` (anything exposing
``.hip_attribution()``), a layer is ``"hidden_states.<l>"`` or the integer ``l``, and there is no autograd fallback.

Differences from Captum 0.7, all stated in ``addvisor_hip/concept.py``: the default classifier is the converged logistic CAV
(``LogisticCAV``), not ``SGDClassifier``; ``save_path`` defaults to None (nothing is written) instead of ``"./cav/"``;
``layer_attr_method`` is a name (``"gradient"``, ``"gradient_x_activation"``, ``"integrated_gradients"``), not a
``LayerAttribution`` object; ``interpret`` also returns the per-input ``"scores"``."""
import re

import torch

from addvisor_hip.concept import CAV, Classifier, Concept, HipTCAV, LogisticCAV, MeanDifferenceCAV, concepts_to_str, tcav_significance

__all__ = ["TCAV", "Concept", "Classifier", "CAV", "LogisticCAV", "MeanDifferenceCAV", "concepts_to_str", "tcav_significance"]


def _layer_index(layer) -> int:
    if isinstance(layer, str):
        m = re.fullmatch(r"hidden_states\.(\d+)", layer)
        if not m:
            raise ValueError(f"a layer name must be 'hidden_states.<l>', not {layer!r}")
        return int(m.group(1))
    if isinstance(layer, bool) or not isinstance(layer, int):
        raise ValueError(f"a layer must be 'hidden_states.<l>' or an integer index into hidden_states, not {layer!r}")
    return layer


class TCAV:
    def __init__(self, model, layers, model_id="default_model_id", classifier=None, layer_attr_method=None,
                 attribute_to_layer_input=False, save_path=None, **classifier_kwargs):
        """``classifier``: None (``LogisticCAV(**classifier_kwargs)``: ``alpha``), ``"mean_difference"``, or an object with the
        ``Classifier`` protocol.  Further ``classifier_kwargs`` go to ``HipTCAV``: ``pool``, ``test_split_ratio``, ``seed``,
        ``internal_batch_size``, ``memory_budget``."""
        if attribute_to_layer_input:
            raise NotImplementedError("TCAV (HIP build) attributes to a layer's output, hidden_states[layer]; "
                                      "attribute_to_layer_input=True is not supported")
        if hasattr(model, "hip_mask_attribution") or not hasattr(model, "hip_attribution"):
            raise TypeError("captum.concept (HIP build) only explains captum_saliency.Wav2vec2LogReg models")
        self.model = model
        self.layers = [layers] if isinstance(layers, (str, int)) else list(layers)
        self._index = {name: _layer_index(name) for name in self.layers}
        self.layer_attr_method = "gradient" if layer_attr_method is None else layer_attr_method
        if classifier is None:
            classifier = LogisticCAV(classifier_kwargs.pop("alpha", 0.01))
        self._engine = HipTCAV(model.hip_attribution(), list(self._index.values()), classifier=classifier, model_id=model_id,
                               save_path=save_path, **classifier_kwargs)

    def _named(self, per_layer: dict) -> dict:
        return {name: per_layer[l] for name, l in self._index.items()}

    def compute_cavs(self, experimental_sets, force_train=False, processes=None):
        return {k: self._named(v) for k, v in self._engine.compute_cavs(experimental_sets, force_train=force_train).items()}

    def interpret(self, inputs, experimental_sets, target=None, additional_forward_args=None, processes=None, **kwargs):
        if additional_forward_args is not None:
            raise NotImplementedError("the classifier takes the waveform alone; additional_forward_args must be None")
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise ValueError("inputs must be a [B, L] waveform tensor")
        out = self._engine.interpret(inputs, experimental_sets, target=target, attr_method=self.layer_attr_method, **kwargs)
        return {k: self._named(v) for k, v in out.items()}
