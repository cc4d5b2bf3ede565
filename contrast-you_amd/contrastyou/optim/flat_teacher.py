"""Flat-buffer teacher of the differentiable mean teacher (semi_seg/hooks/dmt.py).

The hook's deep copy of the model is re-pointed into five flat buffers, so that everything a step does to the teacher's
state costs a constant number of launches or copies whatever the tensor count (about 70 parameter tensors and 44
running statistics for the U-Net):

    data, grad      every parameter and its .grad are views of one f32 buffer each (`FlatParams`)
    stats           every floating-point module buffer (BatchNorm running_mean / running_var)
    counters        every int64 module buffer (num_batches_tracked)
    exp_avg, exp_avg_sq   the Adam moments of the teacher optimizer (torch.optim.Adam of dmt.py:66)

    zero_grad()               one fill
    snapshot() / restore()    three device copies each way: the deepcopy(state_dict()) / load_state_dict of the reference
    perturb(a)                data += a * grad, one cy_axpy (manually_forward_with_grad, dmt.py:22-28)
    adam_step(lr, wd)         one cy_adam_step
    ema_from(student, upd)    EMAUpdater(update_bn=True): one cy_ema_update over the parameters when the student's are
                              slices of one flat buffer in the same order (a FlatOptimizer), else one cy_ema_update_multi;
                              one cy_ema_update_multi over the running statistics

Works on a plain torch.nn model on the GPU as well: there autograd accumulates into the same .grad views.  The Adam
moments are not part of any state dict, as in the reference, whose hook keeps its teacher optimizer out of the
checkpoint.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from cyhip import ops
from cyhip.functions import bump_weights_epoch

from .fused_radam import FlatParams


def _flatten_buffers(bufs: List[torch.Tensor], dtype: torch.dtype, device) -> torch.Tensor:
    """re-point `bufs` into one flat buffer of `dtype`, keeping their values"""
    flat = torch.empty(sum(b.numel() for b in bufs), dtype=dtype, device=device)
    off = 0
    for b in bufs:
        n = b.numel()
        flat[off:off + n].copy_(b.reshape(-1))
        b.data = flat[off:off + n].view(b.shape)
        off += n
    return flat


class FlatTeacher:
    ADAM_BETAS = (0.9, 0.999)  # torch.optim.Adam's defaults, which dmt.py:66 leaves alone
    ADAM_EPS = 1e-8

    def __init__(self, model: nn.Module):
        self.model = model
        self.adam_steps = 0
        self._moments: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._snap: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self._tables = {}  # "params" / "stats" -> (the addresses it was built from, the device table)
        self._build()

    # ---- layout ---------------------------------------------------------------------------------------------------
    def _build(self) -> None:
        params = list(self.model.parameters())
        dev = params[0].device
        self.flat = FlatParams(params)
        named = list(self.model.named_buffers())
        self._float_bufs = [(n, b) for n, b in named if b.is_floating_point()]
        self._int_bufs = [(n, b) for n, b in named if b.dtype == torch.int64]
        assert len(self._float_bufs) + len(self._int_bufs) == len(named), "module buffers are f32 or int64"
        for _, b in self._float_bufs:
            assert b.dtype == torch.float32 and b.device == dev, "flat buffers hold f32 statistics of one device"
        self.stats = _flatten_buffers([b for _, b in self._float_bufs], torch.float32, dev)
        self.counters = _flatten_buffers([b for _, b in self._int_bufs], torch.int64, dev)
        old = self._moments
        self._moments = (torch.zeros_like(self.flat.data), torch.zeros_like(self.flat.data))
        if old is not None:  # the model was moved: the moments follow it
            for new, o in zip(self._moments, old):
                new.copy_(o)
        self._snap = None
        self._tables.clear()
        bump_weights_epoch()

    def _stale(self) -> bool:
        """the model was moved or re-pointed (module.to(device)) after flattening"""
        if self.flat.stale():
            return True
        for flat, bufs in ((self.stats, self._float_bufs), (self.counters, self._int_bufs)):
            lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()
            if any(b.device != flat.device or not (lo <= b.data_ptr() < hi or b.numel() == 0) for _, b in bufs):
                return True
        # (module.to(device) replaces the buffer objects themselves)
        return {id(b) for b in self.model.buffers()} != {id(b) for _, b in self._float_bufs + self._int_bufs}

    def ensure(self) -> "FlatTeacher":
        if self._stale():
            self._build()
        return self

    @property
    def exp_avg(self) -> torch.Tensor:
        return self._moments[0]

    @property
    def exp_avg_sq(self) -> torch.Tensor:
        return self._moments[1]

    # ---- the operations of a step ---------------------------------------------------------------------------------
    def zero_grad(self) -> None:
        if self.flat.grad.is_cuda:
            ops.join_side_streams(torch.cuda.current_stream(self.flat.grad.device))
        self.flat.zero_grad()

    def snapshot(self) -> None:
        """keep the teacher's whole state: parameters, running statistics, batch counters"""
        if self._snap is None:
            self._snap = (torch.empty_like(self.flat.data), torch.empty_like(self.stats),
                          torch.empty_like(self.counters))
        for dst, src in zip(self._snap, (self.flat.data, self.stats, self.counters)):
            dst.copy_(src)

    def restore(self) -> None:
        """put the state of the last snapshot() back"""
        if self._snap is None:
            raise RuntimeError("FlatTeacher.restore() without a snapshot()")
        for dst, src in zip((self.flat.data, self.stats, self.counters), self._snap):
            dst.copy_(src)
        bump_weights_epoch()

    def perturb(self, a: float) -> None:
        """parameters += a * gradients"""
        if self.flat.numel:
            ops.axpy(self.flat.data, self.flat.grad, a)
        bump_weights_epoch()

    def adam_step(self, lr: float, weight_decay: float) -> None:
        """one torch.optim.Adam step over every parameter from the flat gradient (a parameter the backward pass did not
        reach carries a zero gradient, as it does in the reference after its construction-time backward)"""
        self.adam_steps += 1
        if self.flat.numel:
            ops.adam_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq, lr, self.ADAM_BETAS[0],
                          self.ADAM_BETAS[1], self.ADAM_EPS, weight_decay, self.adam_steps)
        bump_weights_epoch()

    def _table(self, key: str, pairs) -> List[torch.Tensor]:
        """the cached device tables (one per 4096 tensors) of `pairs`, rebuilt when an address changed"""
        ptrs = tuple((t.data_ptr(), s.data_ptr()) for t, s in pairs)
        hit = self._tables.get(key)
        if hit is None or hit[0] != ptrs:
            tables = [ops.ema_table(pairs[i:i + ops.EMA_MULTI_MAX], self.flat.data.device)
                      for i in range(0, len(pairs), ops.EMA_MULTI_MAX)]
            hit = self._tables[key] = (ptrs, tables)
        return hit[1]

    def _student_is_flat(self, sp: List[torch.Tensor]) -> bool:
        """the student's parameters are consecutive f32 slices of one buffer, in the teacher's order"""
        if not sp:
            return False
        base = sp[0].data_ptr()
        return all(p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() == base + 4 * off
                   for p, off in zip(sp, self.flat.offsets))

    @torch.no_grad()
    def ema_from(self, student: nn.Module, updater) -> None:
        """EMAUpdater.__call__(ema_model=self.model, student_model=student) with update_bn semantics taken from
        `updater`: its alpha rule, weight decay and step counter"""
        step = updater._global_step
        alpha = min(1 - 1 / (step + 1), updater._alpha) if updater._justify_alpha else updater._alpha
        wd = updater._weight_decay
        sp = [p.data for p in student.parameters()]
        assert len(sp) == len(self.flat.params), (len(sp), len(self.flat.params))
        if self._student_is_flat(sp):
            whole = torch.as_strided(sp[0].reshape(-1), (self.flat.numel,), (1,))
            ops.ema_update(self.flat.data, whole, alpha, wd)
        elif sp:
            pairs = [(t.data, s) for t, s in zip(self.flat.params, sp) if s.numel()]
            for table in self._table("params", pairs):
                ops.ema_update_multi(table, alpha, wd)
        if updater._update_bn:
            mine = dict(self._float_bufs)
            pairs = [(mine[n], b.data) for n, b in student.named_buffers()
                     if ("running_mean" in n or "running_var" in n) and n in mine and b.numel()]
            if pairs:
                for table in self._table("stats", pairs):
                    ops.ema_update_multi(table, alpha, wd)
        bump_weights_epoch()
        updater._global_step += 1
