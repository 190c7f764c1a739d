"""The optimizer tail on the device: AdamW with the clip and the learning-rate schedule inside its step (adamw.py)."""
from .adamw import AdamW, cos_lr_values, reference_param_groups, runner_epoch_values

__all__ = ["AdamW", "cos_lr_values", "runner_epoch_values", "reference_param_groups"]
