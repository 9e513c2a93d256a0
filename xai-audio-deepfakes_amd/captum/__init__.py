"""Minimal ``captum`` stand-in so that ``from captum.attr import Saliency, InputXGradient,
IntegratedGradients`` (captum_saliency.py:3) resolves to the HIP attribution path when this directory is
first on ``sys.path``.  ``captum.attr`` provides the attribution methods the reference names and the
HIP build's further ones; ``captum.metrics`` provides Captum's ``infidelity``, ``sensitivity_max`` and
``infidelity_perturb_func_decorator`` over the same kernels; ``captum.robust`` provides ``FGSM`` and ``PGD`` on the HIP
gradient chain."""
