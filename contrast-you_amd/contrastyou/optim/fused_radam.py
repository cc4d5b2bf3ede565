"""Flat-buffer RAdam: the step is one streaming kernel (cy_radam_step) over the flat buffers of `FlatOptimizer`
(flat_optimizer.py: layout, touched-parameter tracking, data-parallel reduction, checkpoint schema).
Semantics follow torch.optim.RAdam (decoupled_weight_decay=False): see csrc/cy_misc.hip.
Like torch's optimizer, a parameter that received no gradient since the last zero_grad() is
skipped (no weight decay, no moment update, its step count does not advance) -- e.g. the decoder
during encoder pre-training.  "Received a gradient" is tracked per parameter (autograd's
post-accumulate hook, or the kernels' direct accumulation through ops.grad_sink); the step is one
kernel launch per run of consecutive updated parameters with the same step count (normally one).
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch.distributed as dist

from cyhip import ops

from .flat_optimizer import FlatOptimizer, FlatParams  # noqa: F401  (FlatParams: imported from here by its users)


class FusedRAdam(FlatOptimizer):
    """checkpoint schema: {"param_groups", "flat": {group: {step, steps, exp_avg, exp_avg_sq}}}"""

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 process_group: Optional["dist.ProcessGroup"] = None, data_parallel: Optional[bool] = None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults, process_group=process_group, data_parallel=data_parallel)

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _launch(self, g, f, st, a, b, step):
        ops.radam_step(f.data[a:b], f.grad[a:b], st["exp_avg"][a:b], st["exp_avg_sq"][a:b], g["lr"],
                       g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step)
