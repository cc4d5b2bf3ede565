"""Flat-buffer Adam and AdamW: torch.optim.Adam / AdamW(maximize=False) as one launch per run of updated parameters
over the flat buffers of `FlatOptimizer`.  Adam without amsgrad is cy_adam_step (csrc/cy_teacher.hip, the kernel of the
differentiable mean teacher); AdamW and amsgrad are cy_adamw_step (csrc/cy_optim.hip).
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch.distributed as dist

from cyhip import ops

from .flat_optimizer import FlatOptimizer, refuse_flags


class FusedAdam(FlatOptimizer):
    """checkpoint schema: {"param_groups", "flat": {group: {step, steps, exp_avg, exp_avg_sq[, max_exp_avg_sq]}}}"""

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=False, process_group: Optional["dist.ProcessGroup"] = None,
                 data_parallel: Optional[bool] = None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        refuse_flags(maximize=maximize, capturable=capturable, differentiable=differentiable, fused=fused)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad),
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults, process_group=process_group, data_parallel=data_parallel)

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if group["amsgrad"] else ("exp_avg", "exp_avg_sq")

    def _launch(self, g, f, st, a, b, step):
        p, grad, m, v = f.data[a:b], f.grad[a:b], st["exp_avg"][a:b], st["exp_avg_sq"][a:b]
        (b1, b2), decoupled = g["betas"], g["decoupled_weight_decay"]
        if not g["amsgrad"] and not decoupled:
            ops.adam_step(p, grad, m, v, g["lr"], b1, b2, g["eps"], g["weight_decay"], step)
            return
        vmax = None
        if g["amsgrad"]:
            if "max_exp_avg_sq" not in st:  # amsgrad switched on after the buffers were built
                st["max_exp_avg_sq"] = f.data.new_zeros(f.data.shape)
            vmax = st["max_exp_avg_sq"][a:b]
        ops.adamw_step(p, grad, m, v, vmax, g["lr"], b1, b2, g["eps"], g["weight_decay"], decoupled, step)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: Adam with decoupled weight decay, 1e-2 by default"""

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 process_group: Optional["dist.ProcessGroup"] = None, data_parallel: Optional[bool] = None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused,
                         decoupled_weight_decay=True, process_group=process_group, data_parallel=data_parallel)
