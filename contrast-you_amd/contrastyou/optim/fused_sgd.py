"""Flat-buffer SGD: torch.optim.SGD(maximize=False) as one cy_sgd_step launch (csrc/cy_optim.hip) per run of updated
parameters over the flat buffers of `FlatOptimizer`.

A parameter's first update is the one that copies its gradient into the momentum buffer (torch creates the buffer
there): that is the update at its own step count 1, so a parameter that is skipped at first -- no gradient since
zero_grad() -- gets the copy when its first gradient arrives.  Momentum that a scheduler switches on from zero later
starts from a zero buffer.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch.distributed as dist

from cyhip import ops

from .flat_optimizer import FlatOptimizer, refuse_flags


class FusedSGD(FlatOptimizer):
    """checkpoint schema: {"param_groups", "flat": {group: {step, steps, momentum_buffer}}} (no buffer in a group
    without momentum)"""

    def __init__(self, params: Iterable, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *,
                 maximize=False, foreach=None, differentiable=False, fused=None,
                 process_group: Optional["dist.ProcessGroup"] = None, data_parallel: Optional[bool] = None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        refuse_flags(maximize=maximize, differentiable=differentiable, fused=fused)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults, process_group=process_group, data_parallel=data_parallel)

    def _state_names(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _launch(self, g, f, st, a, b, step):
        buf = None
        if g["momentum"] != 0:
            if "momentum_buffer" not in st:  # momentum switched on after the buffers were built
                st["momentum_buffer"] = f.data.new_zeros(f.data.shape)
            buf = st["momentum_buffer"][a:b]
        ops.sgd_step(f.data[a:b], f.grad[a:b], buf, g["lr"], g["momentum"], g["dampening"], g["weight_decay"],
                     g["nesterov"], step == 1)
