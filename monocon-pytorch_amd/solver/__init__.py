"""One-cycle LR / momentum schedule, the fused clip + AdamW step and the fused clip_grad_norm_."""
from .fused_adamw import AdamW, clip_grad_norm_
from .cyclic_scheduler import CyclicScheduler
from .param_groups import build_param_groups

__all__ = ("AdamW", "CyclicScheduler", "clip_grad_norm_", "build_param_groups")
