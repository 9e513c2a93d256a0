"""Captum's ``captum._utils.models`` namespace: only ``linear_model`` is provided."""
