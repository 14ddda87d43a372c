"""One-cycle LR / momentum schedule, the fused clip + AdamW step, the fused clip_grad_norm_, the weight average (ModelEMA)
and gradient accumulation over a window of micro-batches (GradAccumulator)."""
from .fused_adamw import AdamW, clip_grad_norm_
from .cyclic_scheduler import CyclicScheduler
from .param_groups import build_param_groups
from .model_ema import ModelEMA
from .grad_accum import GradAccumulator

__all__ = ("AdamW", "CyclicScheduler", "clip_grad_norm_", "build_param_groups", "ModelEMA", "GradAccumulator")
