"""Captum's ``captum.attr._core`` modules that tutorials import names from directly (``lime``, ``feature_permutation``)."""
