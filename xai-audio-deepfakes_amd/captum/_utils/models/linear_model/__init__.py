"""``captum._utils.models.linear_model``: the interpretable models of Lime (``SkLearnLasso``, ``SkLearnRidge``,
``SkLearnLinearRegression``), solved in float64 on the host without sklearn (addvisor_hip.linear_model states the objectives
and the one difference from Captum's sklearn call: the Lasso runs to a duality gap of 1e-10 instead of 1e-4)."""
from addvisor_hip.linear_model import SkLearnLasso, SkLearnLinearRegression, SkLearnRidge  # noqa: F401
