"""Captum's ``captum._utils`` namespace: only ``models.linear_model`` is provided."""
