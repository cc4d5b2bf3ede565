"""torch.autograd.Function wrappers: the seam between the reference's Python object
protocol (nn.Module blocks, forward hooks, loss objects) and the HIP kernels.

Granularity follows the reference's named blocks (contrastyou/arch/unet.py:16-46): one
Function per _ConvBlock / _UpConv so that `get_module(name)` forward hooks still observe a
block-output tensor with autograd history, while inside a block nothing but raw conv
outputs is materialised (BN+ReLU of conv 1 is applied in conv 2's load path; max-pool,
nearest-upsample and channel concat are addressing modes of the consuming conv).
"""
from __future__ import annotations

import contextlib
import os
from typing import List, Optional

import torch
from torch import Tensor, nn

from . import ops

# bumped by anything that rewrites parameter memory without going through torch
# (fused optimizer, flat-buffer EMA): invalidates the packed-weight cache.
_weights_epoch = 0


# num_batches_tracked counters of the BN layers touched by the current U-Net forward: bumped by
# ONE multi-tensor add at the end of the forward instead of one tiny kernel per BN layer.
_nbt_pending: Optional[list] = None


# running statistics of the BN layers touched by the current U-Net forward (accumulator path, csrc/cy_bn_acc.h): their
# consumers leave the batch moments in memory, ONE launch at the end of the forward blends them into the running buffers
_run_pending: Optional[list] = None


class defer_batch_counters:
    """scope of one network pass: the BatchNorm accumulators of the pass come from one zeroed arena (one fill launch),
    the running statistics and batch counters of its layers are updated by one launch each when the pass ends"""

    def __init__(self, device=None):
        self._device = device

    def __enter__(self):
        global _nbt_pending, _run_pending
        self._outer = (_nbt_pending, _run_pending)
        _nbt_pending, _run_pending = [], []
        self._arena = ops.bn_arena_begin(self._device) if self._device is not None else None
        return self

    def __exit__(self, *exc):
        global _nbt_pending, _run_pending
        pending, running = _nbt_pending, _run_pending
        _nbt_pending, _run_pending = self._outer
        if self._device is not None:
            ops.bn_arena_end(self._arena)
        if exc[0] is None:
            ops.bn_running_update(running)
            if pending:
                with ops.ordered("bn_batch_counters"):
                    torch._foreach_add_(pending, 1)
        return False


# Introspection tap for parity tests (the counterpart of a forward hook for what a block does NOT
# materialise): when set to a callable it receives, for every conv of every block evaluation,
# (bn module, raw conv output y, BN scale, BN shift, materialised block output or None) -- exactly the
# tensors the kernels route ReLU / max-pool decisions by.  None (the default) costs nothing.
RAW_TAP = None


def bump_weights_epoch() -> None:
    global _weights_epoch
    _weights_epoch += 1


def packed_weights(w: Tensor, dtype: torch.dtype):
    """(forward image, dgrad image) of a 3x3 weight, cached ON the parameter object until the
    weight changes.  (A global dict keyed by id(w) would hand a new parameter that reuses a dead
    one's id and storage address the dead one's packed weights.)"""
    tag = (w._version, _weights_epoch, w.data_ptr(), torch.cuda.is_current_stream_capturing())
    cache = w.__dict__.get("_cy_pack")
    if cache is None:
        cache = w.__dict__["_cy_pack"] = {}
    hit = cache.get(dtype)
    cur = torch.cuda.current_stream(w.device)
    if hit is not None and hit[0] == tag:
        # packed on another stream (two-stream forward, side-stream wgrad): wait for it -- unless the
        # event belongs to another graph capture (captures are fenced by full synchronisation)
        if hit[4] != cur and hit[5] == ops._capture_id(cur):
            cur.wait_event(hit[3])
        return hit[1], hit[2]
    wf, wd = ops.pack_weights(w, dtype, want_dgrad=True)
    ev = torch.cuda.Event()
    ev.record(cur)
    cache[dtype] = (tag, wf, wd, ev, cur, ops._capture_id(cur))
    return wf, wd


def prepack(weights, dtype: torch.dtype) -> None:
    """pack ALL the given 3x3 weights with one launch if the first one's packed image is stale (they
    change together, with the optimizer step), and file the results where `packed_weights` looks"""
    if not weights:
        return
    w0 = weights[0]
    cap = torch.cuda.is_current_stream_capturing()
    hit = w0.__dict__.get("_cy_pack", {}).get(dtype)
    if hit is not None and hit[0] == (w0._version, _weights_epoch, w0.data_ptr(), cap):
        return
    cur = torch.cuda.current_stream(w0.device)
    packs = ops.pack_weights_batched([w.detach() for w in weights], dtype)
    ev = torch.cuda.Event()
    ev.record(cur)
    capid = ops._capture_id(cur)
    for w, (wf, wd) in zip(weights, packs):
        w.__dict__.setdefault("_cy_pack", {})[dtype] = ((w._version, _weights_epoch, w.data_ptr(), cap),
                                                        wf, wd, ev, cur, capid)


# ---- weight gradients of a layer that two passes of one step go through ------------------------------
# SemiSupervisedEpocher's two-stage step evaluates the network twice (labeled batch; unlabeled batch +
# its transformed view) and both backward passes add into the same .grad.  Instead of two launches
# (each with its own slab traffic and slab reduction) the pass that reaches a weight FIRST in the
# backward order parks its operands, the second one issues ONE launch over both batches
# (cy_conv3x3_wgrad_pair).  A forward-use counter per weight says whether a partner can still come;
# whatever is still parked when the backward pass ends (the partner's branch got no gradient: e.g. the
# decoder of the unlabeled pass) is issued then as an ordinary single launch.
# Backward passes run in reverse forward order (autograd serves the node with the highest sequence
# number first), so the pass that was evaluated FIRST in a step is differentiated last: it never parks
# -- nobody can come after it -- and takes along what the later passes parked.
PAIR_WGRAD = os.environ.get("CY_PAIR_WGRAD", "1") != "0"
_parked = {}  # id(weight) -> _Parked
_keepalive = []  # operands of joint launches issued from another stream, until the backward pass ends
_pass_serial = 0          # network evaluations so far (begin_pass)
_step_first_pass = None   # serial of the first evaluation since the last backward pass ended


def begin_pass() -> int:
    """called by the network's forward: a new evaluation (pass) begins"""
    global _pass_serial, _step_first_pass
    _pass_serial += 1
    if _step_first_pass is None and torch.is_grad_enabled():  # (evaluation passes are not differentiated)
        _step_first_pass = _pass_serial
        if ops.marks_wanted and torch.cuda.is_available():
            ops.begin_step_marks(torch.cuda.current_device())  # (data parallel: a new step's serial)
    return _pass_serial


class side_pass:
    """`with side_pass():` -- a network evaluation that is differentiated on its own, forward and backward inside the
    block, while another step is between its forward and its backward (the teacher of the differentiable mean teacher,
    inside the student's regularisation).  The pass bookkeeping assumes that one step's passes are differentiated
    together: the enclosing step's first-pass serial is set aside, so that the evaluation inside is the first pass of a
    step of its own and the end of its backward re-arms nothing of the outer step, and put back on the way out."""

    def __enter__(self):
        global _step_first_pass
        self._outer, _step_first_pass = _step_first_pass, None
        return self

    def __exit__(self, *exc):
        global _step_first_pass
        _step_first_pass = self._outer
        return False


class _Parked:
    __slots__ = ("w", "sink", "src1", "src2", "dy", "mode", "scale", "shift", "stream", "event", "capid")


def note_forward_use(w: Tensor, needs_grad: bool) -> None:
    """called by a Function's forward (where grad mode is always off: `needs_grad` comes from
    ctx.needs_input_grad, which is False under an outer no_grad)"""
    if PAIR_WGRAD and needs_grad:
        w.__dict__["_cy_uses"] = w.__dict__.get("_cy_uses", 0) + 1


def _flush_parked() -> None:
    global _step_first_pass
    _step_first_pass = None
    _keepalive.clear()
    for key in list(_parked):
        p = _parked.pop(key)
        p.w.__dict__["_cy_uses"] = 0
        with torch.cuda.stream(p.stream):
            ops.conv3x3_wgrad(p.src1, p.src2, p.dy, mode=p.mode, scale=p.scale, shift=p.shift, out=p.sink, defer=True)
        ops.note_side_work(p.stream)  # (a no-op for the home stream's join; covers a parked side stream)


def wgrad_into_sink(w: Tensor, sink: Tensor, src1: Tensor, src2: Optional[Tensor], dy: Tensor, mode: int,
                    scale: Optional[Tensor], shift: Optional[Tensor], pass_id: int) -> None:
    """sink += dw of one 3x3 conv, pairing the two passes of a step into one launch where it can"""
    uses = w.__dict__.get("_cy_uses", 0)
    if uses > 0:
        # (the step's first pass is differentiated last: whatever the counter still says then -- an
        # evaluation that never reached a loss -- must not leak into the next step)
        uses = 0 if pass_id == _step_first_pass else uses - 1
        w.__dict__["_cy_uses"] = uses
    cur = torch.cuda.current_stream(dy.device)
    p = _parked.pop(id(w), None)
    if p is not None and p.sink is sink and p.mode == mode and p.src1.shape[1:] == src1.shape[1:]:
        if p.stream != cur and p.capid == ops._capture_id(cur):
            cur.wait_event(p.event)
        ops.conv3x3_wgrad_pair(p.src1, p.src2, p.dy, p.scale, p.shift, src1, src2, dy, scale, shift,
                               mode=mode, out=sink, defer=True)
        if p.stream != cur:
            if ops.CAPTURING:
                # inside a capture record_stream is not available: keep the other stream's operands
                # alive until the backward pass (= the capture) ends, so that its allocator cannot hand
                # their memory out again while this launch reads it
                _keepalive.append(p)
            else:
                for t in (p.src1, p.src2, p.dy, p.scale, p.shift):
                    if t is not None:
                        t.record_stream(cur)
        return
    if p is not None:  # not the same layer geometry after all: issue it on its own
        _parked[id(w)] = p
        _flush_parked()
    if PAIR_WGRAD and uses > 0 and pass_id != _step_first_pass and src1.dtype in ops.HALF_TYPES:
        q = _Parked()
        q.w, q.sink, q.src1, q.src2, q.dy, q.mode, q.scale, q.shift = w, sink, src1, src2, dy, mode, scale, shift
        q.stream, q.event, q.capid = cur, torch.cuda.Event(), ops._capture_id(cur)
        q.event.record(cur)
        _parked[id(w)] = q
        ops.at_backward_end(_flush_parked)
        return
    if _step_first_pass is not None:
        ops.at_backward_end(_flush_parked)  # (also re-arms the pass bookkeeping for the next step)
    ops.conv3x3_wgrad(src1, src2, dy, mode=mode, scale=scale, shift=shift, out=sink, defer=True)


def compute_dtype_for(x: Tensor, requested: Optional[torch.dtype]) -> torch.dtype:
    """the requested dtype; else, under autocast (AMPScaler.autocast, contrastyou/amp/amp.py:44), the
    autocast dtype -- float16 in the reference's own mode (fp16 + GradScaler), bfloat16 in the build's
    default mode; else the input's half type; else f32 (verification mode)."""
    if requested is not None:
        return requested
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda")
        return dt if dt in ops.HALF_TYPES else torch.bfloat16
    if x.dtype in ops.HALF_TYPES:
        return x.dtype
    return torch.float32


class ChainCfg:
    """Static description of one [conv3x3 -> BN -> ReLU] x {1,2} block."""

    def __init__(self, bns: List[nn.BatchNorm2d], mode: int, first: bool, pool_out: bool = False):
        self.bns = bns
        self.mode = mode  # ops.CY_SRC_* for the first conv's source 1
        self.first = first  # first conv reads the f32 image (Cin <= 4)
        self.pool_out = pool_out  # second output: MaxPool2d(2) of the block output (written by the same launch)
        # data parallel: when this block's backward has run for the last time in a step, the gradients of every
        # parameter carrying this tag or an earlier one are final (ops.grad_ready_mark)
        self.ready_tag: Optional[str] = None
        self.dtype: Optional[torch.dtype] = None  # forced compute dtype (None = infer)


def _bn_flags(bn: nn.BatchNorm2d, Cout: int):
    """(use_batch, update, on_acc) of one BatchNorm evaluation: batch statistics or the running ones; whether the
    running ones are updated; accumulator path (the consumer derives the coefficients) or finalize launch"""
    use_batch = bn.training or bn.running_mean is None
    update = bn.training and bn.track_running_stats and bn.running_mean is not None
    return use_batch, update, ops.BN_ACC and use_batch and Cout <= 1024


class _BnEval:
    """the BatchNorm evaluation of one conv of a block: the raw conv output `y`; the contiguous coefficient block `coef`
    with rows scale, shift, mean, invstd (and the unbiased variance on the accumulator path), which kernels take by its
    address; `fold`, the ops.BnState whose consumer derives the coefficients (accumulator path), or None when a finalize
    launch wrote them; `batch`: batch statistics, not the running ones; `acc`: the accumulator of the backward sums."""
    __slots__ = ("y", "coef", "fold", "batch", "acc")

    def __init__(self, y: Tensor, coef: Tensor, fold: Optional["ops.BnState"], batch: bool):
        self.y, self.coef, self.fold, self.batch, self.acc = y, coef, fold, batch, None

    @property
    def scale(self) -> Tensor:
        return self.coef[0]

    @property
    def shift(self) -> Tensor:
        return self.coef[1]

    def prologue(self) -> dict:
        """how the conv that reads relu(bn(y)) gets the coefficients: conv3x3_fwd's fold= or its scale= / shift="""
        if self.fold is not None:
            return {"fold": self.fold}
        return {"scale": self.scale, "shift": self.shift}

    def apply(self, pool_out: bool):
        """(relu(bn(y)), its MaxPool2d(2) or None), materialised"""
        if self.fold is not None and pool_out:
            return ops.bn_relu_apply_pool_fold(self.y, self.fold)
        if self.fold is not None:
            return ops.bn_relu_apply_fold(self.y, self.fold), None
        if pool_out:
            return ops.bn_relu_apply_pool(self.y, self.scale, self.shift)
        return ops.bn_relu_apply(self.y, self.scale, self.shift), None

    def tail(self):
        """(y, coef, acc): what a kernel that writes the dA of relu(bn(y)) needs to add the backward sums on the way"""
        return self.y, self.coef, self.acc


def _acc_backward(evals: List[_BnEval]) -> bool:
    """does the block's backward run on accumulators (the finalize-path layers too: they read the first four rows of
    either coefficient block), or on partial rows (CY_BN_ACC=0, or a layer with more than 1024 channels)?"""
    return ops.BN_ACC and all(e.y.shape[1] <= 1024 for e in evals)


# ---- the steps of ConvChainFn.forward ---------------------------------------------------------------------------

def _cast_inputs(cfg: ChainCfg, x1: Tensor, x2: Optional[Tensor], dt: torch.dtype):
    """the block's inputs as its first conv reads them: compute dtype, NHWC (the f32 image of the first layer as is)"""
    if cfg.first:
        return x1, x2
    x1 = ops.to_nhwc(x1 if x1.dtype == dt else x1.to(dt))
    if x2 is not None:
        x2 = ops.to_nhwc(x2 if x2.dtype == dt else x2.to(dt))
    return x1, x2


def _conv_fwd(cfg: ChainCfg, w: Tensor, dt: torch.dtype, src1: Tensor, src2: Optional[Tensor], prev: Optional[_BnEval],
              flags, needs_grad: bool):
    """(y, its statistics) of one conv: the block's first (prev is None) reads the inputs in cfg.mode, a later one
    relu(bn(prev.y)) through its prologue.  The statistics are an accumulator, partial rows or None, as `flags` say."""
    use_batch, _, on_acc = flags
    if prev is None and cfg.first:
        return ops.conv_first_fwd(src1, w, dt, want_stats=use_batch, stats_acc=on_acc)
    note_forward_use(w, needs_grad)
    wf, _ = packed_weights(w, dt)
    if prev is None:
        return ops.conv3x3_fwd(src1, src2, wf, w.shape[0], mode=cfg.mode, want_stats=use_batch, stats_acc=on_acc)
    return ops.conv3x3_fwd(prev.y, None, wf, w.shape[0], want_stats=use_batch, stats_acc=on_acc, **prev.prologue())


def _bn_eval(bn: nn.BatchNorm2d, g: Tensor, b: Tensor, y: Tensor, part, flags, run_items: list) -> _BnEval:
    """the record of bn(y) from the conv's statistics `part`.  Accumulator path: no launch, the consumer of y (the next
    conv's prologue, or the apply launch) derives the coefficients and leaves them in fold.coef; the running statistics
    are an item for `run_items`.  Finalize path: one launch writes the coefficients and the running statistics."""
    use_batch, update, on_acc = flags
    count = y.shape[0] * y.shape[2] * y.shape[3]
    mom = bn.momentum if bn.momentum is not None else 0.1
    if on_acc:
        fold = ops.BnState(part, g.detach(), b.detach(), count, bn.eps, y.device)
        coef = fold.coef
        if update:
            run_items.append((coef, bn.running_mean, bn.running_var, mom))
    else:
        fold = None
        coef = ops.bn_finalize_block(part, count, g.detach(), b.detach(), bn.running_mean, bn.running_var, mom, bn.eps,
                                     use_batch, update, y.shape[1], y.device)
    if update and bn.num_batches_tracked is not None:
        if _nbt_pending is not None:
            _nbt_pending.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    return _BnEval(y, coef, fold, use_batch)


def _running_update(run_items: list) -> None:
    """the running statistics of the block's accumulator-path layers: with the network pass's one launch, or now"""
    if not run_items:
        return
    if _run_pending is not None:
        _run_pending.extend(run_items)
    else:
        ops.bn_running_update(run_items)


def _prepare_backward(ctx, x1: Tensor, x2: Optional[Tensor], evals: List[_BnEval], out: Tensor) -> None:
    """the accumulators of the backward sums, from the same zeroed arena as the forward's (the backward pass allocates
    nothing to zero), and the hand-offs between blocks"""
    cfg = ctx.cfg
    ctx.bwd_accs = None
    if any(ctx.needs_input_grad) and _acc_backward(evals):
        for e in evals:
            e.acc = ops.bn_bwd_acc_new(*e.y.shape, cfg.pool_out and e is evals[-1], e.y.device)
        ctx.bwd_accs = [e.acc for e in evals]
        # whoever produces the gradient of `out` may add the sums of this block's last BatchNorm while it has the
        # values in registers (an _UpConv's upsample backward does): what it needs travels with the tensor
        out._cy_tail = evals[-1].tail()
    # ... and this block, if it upsamples on load, is such a producer for the block whose output it reads
    ctx.up_tail = getattr(x1, "_cy_tail", None) if (cfg.mode == ops.CY_SRC_UP2 and ops.BN_ACC) else None
    ctx.x2_tail = getattr(x2, "_cy_tail", None) if (x2 is not None and ops.BN_ACC) else None


def _save(ctx, x1: Tensor, x2: Optional[Tensor], params, evals: List[_BnEval], out: Optional[Tensor]) -> None:
    """what backward needs: tensors through save_for_backward (x1, [x2], params, (y, coef) per conv, [out]), the rest
    of the records by attribute.  `_saved` is the other half: nobody else knows the order."""
    # (the coefficients of an accumulator-path layer exist once a consumer of y has derived them)
    assert all(e.fold is None or e.fold.done for e in evals), "BatchNorm coefficients no consumer has written"
    ctx.has_x2 = x2 is not None
    ctx.batch_flags = [e.batch for e in evals]
    tensors = [x1] + ([x2] if x2 is not None else []) + list(params)
    for e in evals:
        tensors += (e.y, e.coef)
    if out is not None:
        tensors.append(out)
    ctx.save_for_backward(*tensors)


def _saved(ctx):
    """(x1, x2 or None, params, records, out or None) as `_save` filed them; the records' accumulators come from
    `_backward_accs`"""
    t = ctx.saved_tensors
    n, k = ctx.nconv, 2 if ctx.has_x2 else 1
    evals = [_BnEval(t[k + 3 * n + 2 * i], t[k + 3 * n + 2 * i + 1], None, ctx.batch_flags[i]) for i in range(n)]
    return t[0], (t[1] if ctx.has_x2 else None), t[k:k + 3 * n], evals, (t[-1] if ctx.cfg.pool_out else None)


# ---- the steps of ConvChainFn.backward --------------------------------------------------------------------------

def _backward_accs(ctx, evals: List[_BnEval]) -> bool:
    """is this backward on accumulators (`_acc_backward`)?  If so the records get the ones the forward took (a second
    backward through the same node: none, fresh ones are taken where needed)."""
    accs, ctx.bwd_accs = ctx.bwd_accs, None
    if not _acc_backward(evals):
        return False
    if accs is not None:
        for e, acc in zip(evals, accs):
            e.acc = acc
    return True


def _pooled_grad(out: Tensor, dout: Optional[Tensor], dpooled: Tensor, ev: _BnEval, on_acc: bool):
    """(dA of the block's last BatchNorm, its partial rows or None) when the block also wrote MaxPool2d(2) of its
    output: the pooled branch's gradient through the arg-max of `out` plus the skip branch's `dout`.  The same launch
    adds that BatchNorm's backward sums: into its accumulator while vacant (BnAccBuf's rule), else into a fresh one;
    as partial rows on the partial-row path."""
    if dpooled.dtype != out.dtype:
        dpooled = dpooled.to(out.dtype)
    add = None if dout is None else ops.to_nhwc(dout if dout.dtype == out.dtype else dout.to(out.dtype))
    if not on_acc:
        return ops.maxpool2_bwd_bn(out, ops.to_nhwc(dpooled), add, ev.y, *ev.coef[:4])
    acc = ev.acc if ev.acc is not None and ev.acc.vacant() else None
    da, acc = ops.maxpool2_bwd_bn_acc(out, ops.to_nhwc(dpooled), add, ev.y, ev.coef, acc)
    if acc is not None:
        acc.filled(da)
        ev.acc = acc
    return da, None


def _bn_relu_grad(ctx, i: int, da: Tensor, params, ev: _BnEval, on_acc: bool, partials: Optional[Tensor],
                  split: Optional[int]):
    """backward of relu(bn(y)) of conv i at `da`: (data gradient of the conv or None, dy, dgamma, dbeta).  The
    BatchNorm's backward sums come from partial rows (legacy path) or an accumulator: a producer's, if it holds the sums
    of exactly `da` (BnAccBuf's rule), else the reduce launch's.  Where the layer has a launch plan for it, the data
    gradient takes the BatchNorm + ReLU backward into its load path (conv3x3_dgrad_bn: one launch instead of two)."""
    need = ctx.needs_input_grad
    w, g, b = params[3 * i: 3 * i + 3]
    need_g, need_b = need[4 + 3 * i], need[5 + 3 * i]
    # parameter gradients are accumulated straight into .grad when it is a live f32 buffer (flat-buffer optimizer);
    # otherwise they are returned to autograd as usual
    gsink = ops.grad_sink(g) if (need_g and need_b) else None
    bsink = ops.grad_sink(b) if gsink is not None else None
    pgrads = dict(dgamma_out=gsink if bsink is not None else None, dbeta_out=bsink, want_param_grads=need_g or need_b)
    y = ev.y
    if not on_acc:
        return (None, *ops.bn_relu_bwd(da, y, *ev.coef[:4], ev.batch, partials=partials, **pgrads))
    acc, done = ops.bn_acc_for_grad(ev.acc, da, y)
    if i > 0 or (not ctx.cfg.first and (need[1] or (ctx.has_x2 and need[2]))):
        da_f = ops.to_nhwc(da if da.dtype == y.dtype else da.to(y.dtype))
        if ops.conv3x3_dgrad_bn_ok(da_f, w.shape[1], split):
            acc = acc if acc is not None else ops.bn_bwd_acc_new(*y.shape, False, y.device)
            if not done:
                ops.bn_bwd_reduce_acc(da_f, y, ev.coef, acc)
            _, wd = packed_weights(w, ctx.dt)
            return ops.conv3x3_dgrad_bn(da_f, y, ev.coef, acc, ev.batch, wd, w.shape[1], split=split, **pgrads)
    return (None, *ops.bn_relu_bwd_acc(da, y, ev.coef, ev.batch, acc=acc, acc_filled=done, **pgrads))


def _weight_grad(w: Tensor, sink: Optional[Tensor], src1: Tensor, src2: Optional[Tensor], dy: Tensor, mode: int,
                 scale: Optional[Tensor], shift: Optional[Tensor], first: bool, pass_id: int) -> Optional[Tensor]:
    """dw of one 3x3 conv (of the image-reading first layer if `first`): added into the live .grad `sink` -- on the side
    stream with ASYNC_WGRAD, its slab sum deferred to the batched launch of the backward pass (ops.DEFER_WGRAD_REDUCE)
    -- and None returned, or returned"""
    side = sink is not None and ops.ASYNC_WGRAD
    with ops.on_side_stream(src1, src2, dy, scale, shift) if side else contextlib.nullcontext():
        if first:
            dw = ops.conv_first_wgrad(src1, dy, out=sink, defer=sink is not None)
        elif sink is not None:
            wgrad_into_sink(w, sink, src1, src2, dy, mode, scale, shift, pass_id)
        else:
            dw = ops.conv3x3_wgrad(src1, src2, dy, mode=mode, scale=scale, shift=shift)
    return None if sink is not None else dw


def _data_grad(w: Tensor, wd: Tensor, dy: Tensor, split: Optional[int], tail):
    """conv3x3 data gradient of dy; with `split`, the two parts of a concatenated input.  tail = (y, coef, acc): the
    output (its second part when split) is the dA of relu(bn(y)); where the launch plan allows, the epilogue adds that
    BatchNorm's backward sums into acc while vacant (BnAccBuf's rule)."""
    Cin, c0 = w.shape[1], split or 0
    if tail is not None and tail[2].vacant() and ops.conv3x3_dgrad_dz_ok(dy, Cin, split, c0, Cin - c0):
        dx = ops.conv3x3_dgrad_dz(dy, wd, Cin, *tail, split=split)
        tail[2].filled(dx[1] if split else dx)
        return dx
    return ops.conv3x3_fwd(dy, None, wd, Cin, want_stats=False, split=split)[0]


def _upsample_grad(dup: Tensor, tail) -> Tensor:
    """gradient through the nearest 2x upsample.  tail = (y, coef, acc) of the block that produced the upsampled input:
    the result is the dA of its relu(bn(y)), and the same launch adds those backward sums into acc while vacant."""
    if tail is not None and tail[2].vacant():
        dx = ops.upsample2_bwd_bn_acc(dup, *tail)
        if dx is not None:
            tail[2].filled(dx)
            return dx
    return ops.upsample2_bwd(dup)


def _input_grads(ctx, x1: Tensor, w: Tensor, dy: Tensor, fused_dx):
    """(dx1, dx2) from dy of the block's first conv, or from the data gradient the fused launch already made: x1's
    through the 2x2 max-pool or the upsample the conv reads it with, or directly; x2's (a concat input) directly"""
    cfg, need = ctx.cfg, ctx.needs_input_grad
    need_x1, need_x2 = need[1], ctx.has_x2 and need[2]
    if not (need_x1 or need_x2):
        return None, None
    if cfg.first:
        raise RuntimeError("gradient w.r.t. the input image is not implemented (the reference never asks for it)")
    _, wd = packed_weights(w, ctx.dt)
    dl = fused_dx if fused_dx is not None else \
        _data_grad(w, wd, dy, x1.shape[1] if ctx.has_x2 else None, ctx.x2_tail if need_x2 else None)
    dl1, dl2 = dl if ctx.has_x2 else (dl, None)
    dx2 = dl2 if need_x2 else None
    if not need_x1:
        return None, dx2
    if cfg.mode == ops.CY_SRC_POOL2:
        dx1 = ops.maxpool2_bwd(x1, dl1)
    elif cfg.mode == ops.CY_SRC_UP2:
        dx1 = _upsample_grad(dl1, ctx.up_tail)
    else:
        dx1 = dl1
    return (dx1 if dx1.dtype == ctx.x_dtype else dx1.to(ctx.x_dtype)), dx2


class ConvChainFn(torch.autograd.Function):
    """One reference block: _ConvBlock (2 convs) or _UpConv (upsample + 1 conv)."""

    @staticmethod
    def forward(ctx, cfg: ChainCfg, x1: Tensor, x2: Optional[Tensor], *params: Tensor):
        nconv = len(params) // 3
        ops.require_gpu(x1, x2, *params)
        dt = compute_dtype_for(x1, cfg.dtype)
        ctx.cfg, ctx.nconv, ctx.dt = cfg, nconv, dt
        ctx.pass_id = _pass_serial
        ctx.x_dtype = x1.dtype
        x1s, x2s = _cast_inputs(cfg, x1, x2, dt)
        evals: List[_BnEval] = []
        run_items = []
        for i in range(nconv):
            w, g, b = params[3 * i: 3 * i + 3]
            flags = _bn_flags(cfg.bns[i], w.shape[0])
            y, part = _conv_fwd(cfg, w, dt, x1s, x2s, evals[-1] if evals else None, flags,
                                ctx.needs_input_grad[3 + 3 * i])
            evals.append(_bn_eval(cfg.bns[i], g, b, y, part, flags, run_items))
        out, pooled = evals[-1].apply(cfg.pool_out)
        _running_update(run_items)
        _prepare_backward(ctx, x1, x2, evals, out)
        if cfg.pool_out:
            # backward of the pooled output routes through the arg-max of `out`; either output may go unused
            # (a pass whose loss taps only the encoder leaves `out`'s skip branch without a gradient)
            ctx.set_materialize_grads(False)
        _save(ctx, x1s, x2s, params, evals, out if cfg.pool_out else None)
        if RAW_TAP is not None:
            for bn, e in zip(cfg.bns, evals):
                RAW_TAP(bn, e.y, e.scale, e.shift, out if e is evals[-1] else None)
        return (out, pooled) if cfg.pool_out else out

    @staticmethod
    def backward(ctx, dout: Optional[Tensor], dpooled: Optional[Tensor] = None):
        ops.ensure_backward_join()
        cfg, nconv, need = ctx.cfg, ctx.nconv, ctx.needs_input_grad  # (need: cfg, x1, x2, *params)
        x1, x2, params, evals, out = _saved(ctx)
        if cfg.pool_out and dout is None and dpooled is None:
            return (None,) * (3 + 3 * nconv)
        on_acc = _backward_accs(ctx, evals)
        da, partials = dout, None
        if cfg.pool_out and dpooled is not None:
            da, partials = _pooled_grad(out, dout, dpooled, evals[-1], on_acc)
        grads_p: List[Optional[Tensor]] = [None] * (3 * nconv)
        for i in reversed(range(nconv)):
            w = params[3 * i]
            prev = evals[i - 1] if i > 0 else None
            fused_dx, dy, dgamma, dbeta = _bn_relu_grad(ctx, i, da, params, evals[i], on_acc,
                                                        partials if i == nconv - 1 else None,
                                                        x1.shape[1] if (i == 0 and ctx.has_x2) else None)
            grads_p[3 * i + 1] = dgamma if need[4 + 3 * i] else None
            grads_p[3 * i + 2] = dbeta if need[5 + 3 * i] else None
            if need[3 + 3 * i] and prev is not None:
                grads_p[3 * i] = _weight_grad(w, ops.grad_sink(w), prev.y, None, dy, 0, prev.scale, prev.shift, False,
                                              ctx.pass_id)
            elif need[3 + 3 * i]:
                grads_p[3 * i] = _weight_grad(w, ops.grad_sink(w), x1, x2, dy, cfg.mode, None, None, cfg.first,
                                              ctx.pass_id)
            if prev is not None:
                tail = prev.tail() if prev.acc is not None else None
                da = fused_dx if fused_dx is not None else _data_grad(w, packed_weights(w, ctx.dt)[1], dy, None, tail)
        dx1, dx2 = _input_grads(ctx, x1, params[0], dy, fused_dx)
        if cfg.ready_tag is not None and (_step_first_pass is None or ctx.pass_id == _step_first_pass):
            # (the pass evaluated first is differentiated last: nothing of this block is parked or still to come)
            ops.grad_ready_mark(cfg.ready_tag, dy.device)
        return (None, dx1, dx2, *grads_p)


class HeadFn(torch.autograd.Function):
    """nn.Conv2d(C, K, 1) with bias (contrastyou/arch/unet.py:102); f32 logits."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Optional[Tensor]):
        ops.require_gpu(x, w)
        x = ops.to_nhwc(x)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.bias = b  # the parameter object (for its .grad sink), not saved data
        return ops.head_fwd(x, w, b)

    @staticmethod
    def backward(ctx, dlogits: Tensor):
        x, w = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (
            ctx.has_bias and ctx.needs_input_grad[2])
        # like the conv / BN parameters: the reduction kernel adds straight into live .grad buffers (ordered across
        # streams), so that autograd never has to merge the two passes' contributions itself
        wsink = ops.grad_sink(w) if (need_dw and ctx.needs_input_grad[1] and w.dtype == torch.float32) else None
        bsink = ops.grad_sink(ctx.bias) if (wsink is not None and ctx.has_bias and ctx.needs_input_grad[2]) else None
        if wsink is not None and (bsink is not None or not ctx.has_bias):
            dx, _, _ = ops.head_bwd(x, w, dlogits, need_dx, True, dw_into=wsink, db_into=bsink)
            return dx, None, None
        dx, dw, db = ops.head_bwd(x, w, dlogits, need_dx, need_dw)
        if dw is not None:
            dw = dw.to(w.dtype)
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.has_bias else None


class SoftmaxKLFn(torch.autograd.Function):
    """KL_div(softmax(logits,1), one_hot(target)) with mean reduction
    (semi_seg/epochers/epocher.py:317-318, contrastyou/losses/kl.py:112-125)."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, eps: float):
        ops.require_gpu(logits, target)
        logits = ops.to_nhwc(logits.float())
        target = target.contiguous()
        ctx.save_for_backward(logits, target)
        ctx.eps = eps
        return ops.softmax_kl_fwd(logits, target, eps)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_kl_bwd(logits, target, gs, ctx.eps), None, None


class SoftmaxWeightedKLFn(torch.autograd.Function):
    """KL_div(weight=w, reduction=reduction)(softmax(logits,1), one_hot(target)) for any class weights (`weight`: the
    normalised [K] f32 device tensor, or None) and any of the three reductions (contrastyou/losses/kl.py:94-125);
    "none" returns the [N, H, W] map."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, weight: Optional[Tensor], eps: float, reduction: str):
        ops.require_gpu(logits, target, weight)
        logits = ops.to_nhwc(logits.float())
        target = target.contiguous()
        ctx.save_for_backward(logits, target)
        ctx.weight, ctx.eps, ctx.reduction = weight, eps, reduction
        return ops.softmax_wkl_fwd(logits, target, weight, eps, reduction)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target = ctx.saved_tensors
        up = g.float().contiguous() if ctx.reduction == "none" else g.reshape(1).float().contiguous()
        return ops.softmax_wkl_bwd(logits, target, ctx.weight, up, ctx.eps, ctx.reduction), None, None, None, None


class SoftmaxDiceFn(torch.autograd.Function):
    """DiceLoss(ignore_index=ignore, smooth=smooth, p=p, reduction=reduction)(softmax(logits,1), one_hot(target)) for
    p in {1, 2} (contrastyou/losses/dice_loss.py:46-105); "none" returns the [N] vector.  The forward's [N, K] table of
    numerators and denominators is kept for the backward."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, p: int, smooth: float, ignore: Optional[int], reduction: str):
        ops.require_gpu(logits, target)
        logits = ops.to_nhwc(logits.float())
        target = target.contiguous()
        res, table = ops.softmax_dice_fwd(logits, target, p, smooth, ignore, reduction)
        ctx.save_for_backward(logits, target, table)
        ctx.p, ctx.ignore, ctx.reduction = p, ignore, reduction
        return res

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target, table = ctx.saved_tensors
        up = g.reshape(-1).float().contiguous()
        return ops.softmax_dice_bwd(logits, target, table, up, ctx.p, ctx.ignore, ctx.reduction), None, None, None, \
            None, None


class SoftmaxGroupKLFn(torch.autograd.Function):
    """MultiCoreKL(grouper(range(K), G))(softmax(logits,1), one_hot(target, G)): KL_div of the per-class sums of the
    softmax over K/G contiguous channels, mean reduction (contrastyou/losses/multicore_loss.py:41-60)."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, G: int, eps: float):
        ops.require_gpu(logits, target)
        logits = ops.to_nhwc(logits.float())
        target = target.contiguous()
        ctx.save_for_backward(logits, target)
        ctx.G, ctx.eps = G, eps
        return ops.softmax_group_kl_fwd(logits, target, G, eps)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_group_kl_bwd(logits, target, gs, ctx.G, ctx.eps), None, None, None


class SoftmaxMixKLFn(torch.autograd.Function):
    """KL_div(softmax(logits,1) mixed by `mix` [K, C], one_hot(target, C)), mean reduction: the KL term of the adaptive
    over-segmented criteria (contrastyou/losses/multicore_loss.py:63-149).  Gradients go to the logits and, where it
    asks for one, to `mix` (one more launch)."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, mix: Tensor, eps: float):
        ops.require_gpu(logits, target, mix)
        logits = ops.to_nhwc(logits.float())
        target = target.contiguous()
        mix = mix.detach().float().contiguous()
        ctx.save_for_backward(logits, target, mix)
        ctx.eps = eps
        return ops.softmax_mix_kl_fwd(logits, target, mix, eps)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target, mix = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        dlogits, dmix = ops.softmax_mix_kl_bwd(logits, target, mix, gs, ctx.eps, ctx.needs_input_grad[2])
        return dlogits, None, dmix, None


class SoftmaxMSEFn(torch.autograd.Function):
    """nn.MSELoss()(a.softmax(1), b.softmax(1)) (semi_seg/hooks/consistency.py:36, mt.py:186)."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        ops.require_gpu(a, b)
        a = ops.to_nhwc(a.float())
        b = ops.to_nhwc(b.float())
        ctx.save_for_backward(a, b)
        return ops.softmax_mse_fwd(a, b)

    @staticmethod
    def backward(ctx, g: Tensor):
        a, b = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        da, db = ops.softmax_mse_bwd(a, b, gs, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return da, db


class MixupKLFn(torch.autograd.Function):
    """KL_div(eps=eps)(logits.softmax(1), w_self * onehot(target) + w_other * onehot(target)[index]), mean reduction
    (semi_seg/hooks/mixup.py:49-58 with mixup_data of hooks/utils.py:284-297).  target: integer labels [N,H,W] or
    [N,1,H,W]; index: a CPU integer tensor [N] (or its ops.mix_index copy).  Neither one-hot tensor is formed."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, index: Tensor, w_self: float, w_other: float, eps: float = 1e-16):
        ops.require_gpu(logits, target)
        logits = ops.to_nhwc(logits.float())
        N, _, H, W = logits.shape
        target = target.reshape(N, H, W).to(torch.int64).contiguous()
        index = ops.mix_index(index, N, logits.device)
        ctx.save_for_backward(logits, target, index)
        ctx.args = (float(w_self), float(w_other), float(eps))
        return ops.softmax_mixkl_fwd(logits, target, index, *ctx.args)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, target, index = ctx.saved_tensors
        w_self, w_other, eps = ctx.args
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_mixkl_bwd(logits, target, index, w_self, w_other, gs, eps), None, None, None, None, None


class MixSoftmaxMSEFn(torch.autograd.Function):
    """MSELoss(reduction="none")(student.softmax(1), w_self * teacher.softmax(1) + w_other * teacher.softmax(1)[index])
    .mean() (semi_seg/hooks/mt.py:301-319).  The gradient goes to the student alone; the mixed target lives in
    registers.  Up to 64 classes (past 16: csrc/cy_wide_reg.hip)."""

    @staticmethod
    def forward(ctx, student_logits: Tensor, teacher_logits: Tensor, index: Tensor, w_self: float, w_other: float):
        ops.require_gpu(student_logits, teacher_logits)
        student = ops.to_nhwc(student_logits.float())
        teacher = ops.to_nhwc(teacher_logits.detach().float())
        index = ops.mix_index(index, student.shape[0], student.device)
        ctx.save_for_backward(student, teacher, index)
        ctx.args = (float(w_self), float(w_other))
        return ops.softmax_mixmse_fwd(student, teacher, index, *ctx.args)

    @staticmethod
    def backward(ctx, g: Tensor):
        student, teacher, index = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_mixmse_bwd(student, teacher, index, *ctx.args, gs), None, None, None, None


class SoftmaxGatherMSEFn(torch.autograd.Function):
    """nn.MSELoss()(warp(teacher.softmax(1)), student.softmax(1)), the consistency term of the differentiable mean
    teacher (semi_seg/hooks/dmt.py:138-146): the teacher's PROBABILITIES go through the nearest-neighbour affine map
    with zero padding, so a pixel warped in from outside the image carries the all-zero vector (SoftmaxMSEFn on warped
    logits would give it the uniform softmax of zero logits).  `teacher_logits` are unwarped; `source_map` is the int32
    [N,H,W] map of ops.source_map_from_warped.  The gradient goes to the student alone; neither softmax, nor the warped
    tensor, nor the difference is formed."""

    @staticmethod
    def forward(ctx, teacher_logits: Tensor, source_map: Tensor, student_logits: Tensor):
        ops.require_gpu(teacher_logits, source_map, student_logits)
        student = ops.to_nhwc(student_logits.float())
        teacher = ops.to_nhwc(teacher_logits.detach().float())
        ctx.save_for_backward(teacher, source_map, student)
        return ops.softmax_gathermse_fwd(teacher, source_map, student)

    @staticmethod
    def backward(ctx, g: Tensor):
        teacher, source_map, student = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return None, None, ops.softmax_gathermse_bwd(teacher, source_map, student, gs)


class DAELossFn(torch.autograd.Function):
    """F.mse_loss(act(conv1x1(logits)), image) with the 1x1 convolution K -> 1 of weight [1,K,1,1] (or [K]) and bias
    [1], act "sigmoid" or "tanh" (semi_seg/hooks/autoencoder.py:52-57).  Gradients go to the logits, the weight and
    the bias, none to the image.  One pass over the logits each way; no reconstruction or difference map is formed.
    A contiguous f32 image -- the one-channel input of the U-Net -- is read in place."""

    @staticmethod
    def forward(ctx, logits: Tensor, weight: Tensor, bias: Tensor, image: Tensor, activation: str = "sigmoid"):
        ops.require_gpu(logits, weight, bias, image)
        if activation not in ops.PRIOR_ACTS:
            raise ValueError(f"activation must be 'sigmoid' or 'tanh', got {activation!r}")
        K = logits.shape[1]
        if weight.numel() != K or bias.numel() != 1:
            raise ValueError(f"the fused DAE loss reconstructs one channel: expected a weight of {K} elements and a "
                             f"bias of 1, got {tuple(weight.shape)} and {tuple(bias.shape)}")
        logits = ops.to_nhwc(logits.float())
        image = image.detach().float().contiguous()
        w, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        ctx.save_for_backward(logits, w, b, image)
        ctx.act = ops.PRIOR_ACTS[activation]
        ctx.shapes = (weight.shape, bias.shape, weight.dtype, bias.dtype)
        return ops.dae_fwd(logits, w, b, image, ctx.act)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, w, b, image = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        d, dw, db = ops.dae_bwd(logits, w, b, image, ctx.act, gs)
        wshape, bshape, wdt, bdt = ctx.shapes
        return d, dw.view(wshape).to(wdt), db.view(bshape).to(bdt), None, None


class OrthoLossFn(torch.autograd.Function):
    """((n n^T - I)^2).mean() with n = F.normalize(prototypes) (semi_seg/hooks/orthogonal.py:45-50): prototypes [K, C]
    or [K, C, 1, 1], 2 <= K <= 64, K * C <= 16384.  One launch each way; the backward recomputes n and the Gram matrix.
    Where the prototypes are a parameter with a live f32 .grad buffer (the flat buffers of FusedRAdam), the gradient
    is added there in the order of the head's own weight gradient (`ops.ordered`), as the kernels of the network do:
    autograd's own accumulation would not be ordered against a weight-gradient kernel of another stream."""

    @staticmethod
    def forward(ctx, prototypes: Tensor):
        ops.require_gpu(prototypes)
        if not (prototypes.dim() == 2 or (prototypes.dim() == 4 and tuple(prototypes.shape[2:]) == (1, 1))):
            raise ValueError(f"prototypes must be [K, C] or [K, C, 1, 1], got {tuple(prototypes.shape)}")
        v = prototypes.detach().float().reshape(prototypes.shape[0], prototypes.shape[1]).contiguous()
        ctx.save_for_backward(v)
        ctx.param = prototypes  # the parameter object (for its .grad sink), not saved data
        return ops.ortho_fwd(v)

    @staticmethod
    def backward(ctx, g: Tensor):
        (v,) = ctx.saved_tensors
        p = ctx.param
        d = ops.ortho_bwd(v, g.reshape(1).float().contiguous()).view(p.shape)
        sink = ops.grad_sink(p) if p.dtype == torch.float32 else None
        if sink is not None:
            with ops.ordered(("head_grad", sink.data_ptr())):
                sink.add_(d)
            return None
        return d.to(p.dtype)


class SoftmaxEntropyFn(torch.autograd.Function):
    """Entropy(eps=eps)(logits.softmax(1)), mean reduction (semi_seg/hooks/entmin.py:29-30,
    contrastyou/losses/kl.py:48-56).  Up to 64 classes (past 16: csrc/cy_wide_reg.hip)."""

    @staticmethod
    def forward(ctx, logits: Tensor, eps: float):
        ops.require_gpu(logits)
        logits = ops.to_nhwc(logits.float())
        ctx.save_for_backward(logits)
        ctx.eps = eps
        return ops.softmax_entropy_fwd(logits, eps)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_entropy_bwd(logits, gs, ctx.eps), None


class SoftmaxSelfMSEFn(torch.autograd.Function):
    """nn.MSELoss()(p, one_hot(p.max(1)[1])) with p = logits.softmax(1); the one-hot carries no gradient and is never
    materialised (semi_seg/hooks/pseudolabel.py:30-36).  Up to 64 classes (past 16: csrc/cy_wide_reg.hip)."""

    @staticmethod
    def forward(ctx, logits: Tensor):
        ops.require_gpu(logits)
        logits = ops.to_nhwc(logits.float())
        ctx.save_for_backward(logits)
        return ops.softmax_selfmse_fwd(logits)

    @staticmethod
    def backward(ctx, g: Tensor):
        logits, = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.softmax_selfmse_bwd(logits, gs)


class UAMTLossFn(torch.autograd.Function):
    """(loss, mask_mean) of the uncertainty-aware mean teacher (semi_seg/hooks/mt.py:242-248,266-267): the MSE of
    softmax(teacher) [hard: its arg-max one-hot] and softmax(student) over the pixels whose teacher entropy lies below
    `thr`, over (mask_mean + 1e-2).  Both stay on the device; mask_mean is not differentiable, the teacher gets no
    gradient.  Up to 64 classes (past 16: csrc/cy_wide_reg.hip)."""

    @staticmethod
    def forward(ctx, teacher_logits: Tensor, student_logits: Tensor, thr: float, hard: bool):
        ops.require_gpu(teacher_logits, student_logits)
        if teacher_logits.shape != student_logits.shape:
            raise ValueError(f"teacher {tuple(teacher_logits.shape)} and student {tuple(student_logits.shape)} differ")
        t = ops.to_nhwc(teacher_logits.detach().float())
        s = ops.to_nhwc(student_logits.float())
        res = ops.uamt_mse_fwd(t, s, thr, hard)
        ctx.save_for_backward(t, s, res)
        ctx.thr, ctx.hard = float(thr), bool(hard)
        loss, mask_mean = res[0], res[1]
        ctx.mark_non_differentiable(mask_mean)
        return loss, mask_mean

    @staticmethod
    def backward(ctx, g: Tensor, _g_mask):
        t, s, res = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return None, ops.uamt_mse_bwd(t, s, res, gs, ctx.thr, ctx.hard), None, None


class AvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d((1,1)) + Flatten (contrastyou/projectors/heads.py:15-16)."""

    @staticmethod
    def forward(ctx, x: Tensor):
        ops.require_gpu(x)
        x = ops.to_nhwc(x)
        ctx.shape, ctx.dtype = tuple(x.shape), x.dtype
        return ops.avgpool_fwd(x)

    @staticmethod
    def backward(ctx, g: Tensor):
        return ops.avgpool_bwd(g.float().contiguous(), ctx.shape, ctx.dtype)


class LinearFn(torch.autograd.Function):
    """nn.Linear (+ optional in-place LeakyReLU), contrastyou/projectors/heads.py:17-19."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Optional[Tensor], act: int, slope: float):
        ops.require_gpu(x, w)
        x = x.float().contiguous()
        w32 = w.detach().float().contiguous()
        y = ops.linear_fwd(x, w32, None if b is None else b.detach().float().contiguous(), act, slope)
        ctx.save_for_backward(x, w32, y)
        ctx.act, ctx.slope, ctx.has_bias = act, slope, b is not None
        ctx.params = (w, b)  # (leaf parameters: their .grad buffers take the gradients directly when they can)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w, y = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dw = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        wp, bp = ctx.params
        wsink = bsink = None
        if ctx.needs_input_grad[1] and (not ctx.has_bias or ctx.needs_input_grad[2]):
            wsink = ops.grad_sink(wp)
            bsink = ops.grad_sink(bp) if ctx.has_bias and wsink is not None else None
            if ctx.has_bias and bsink is None:
                wsink = None
        dx, dw, db = ops.linear_bwd(x, w, y, g.float().contiguous(), ctx.act, ctx.slope, need_dx,
                                    need_dw, dw_into=wsink, db_into=bsink)
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.has_bias else None, None, None


class ProjHeadFn(torch.autograd.Function):
    """ProjectionHead, head_type "mlp" with normalisation, as ONE launch forward and two backward
    (contrastyou/projectors/heads.py:12-22,81-96): pool -> Linear -> LeakyReLU(0.01) -> Linear -> F.normalize."""

    @staticmethod
    def forward(ctx, x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor):
        ops.require_gpu(x, w1, w2)
        x = ops.to_nhwc(x)
        z, pooled, y1, y2, norms = ops.proj_head_fwd(x, w1.detach().float().contiguous(), b1.detach().float().contiguous(),
                                                     w2.detach().float().contiguous(), b2.detach().float().contiguous())
        ctx.save_for_backward(pooled, y1, y2, norms, w1.detach(), w2.detach())
        ctx.shape, ctx.dtype = tuple(x.shape), x.dtype
        ctx.params = (w1, b1, w2, b2)
        return z

    @staticmethod
    def backward(ctx, g: Tensor):
        pooled, y1, y2, norms, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        sinks = None
        if all(need[1:5]):
            cand = tuple(ops.grad_sink(p) for p in ctx.params)
            if all(c is not None for c in cand):
                sinks = cand
        dx, (dw1, db1, dw2, db2) = ops.proj_head_bwd(g.float().contiguous(), pooled, y1, y2, norms,
                                                     w1.float().contiguous(), w2.float().contiguous(), ctx.shape,
                                                     ctx.dtype, need[0], sinks)
        return (dx, dw1 if need[1] else None, db1 if need[2] else None, dw2 if need[3] else None,
                db2 if need[4] else None)


class L2NormFn(torch.autograd.Function):
    """F.normalize(x, p=2, dim=1) on [M,D] (contrastyou/projectors/nn.py:47-54)."""

    @staticmethod
    def forward(ctx, x: Tensor):
        ops.require_gpu(x)
        x = x.float().contiguous()
        z, norms = ops.l2norm_fwd(x)
        ctx.save_for_backward(x, norms)
        return z

    @staticmethod
    def backward(ctx, g: Tensor):
        x, norms = ctx.saved_tensors
        return ops.l2norm_bwd(x, norms, g.float().contiguous())


class SupConFn(torch.autograd.Function):
    """SupConLoss1._forward (contrastyou/losses/contrastive.py:52-100) on P = cat(z1, z2).  Returns the loss, the
    diagonal of the similarity matrix (|P_i|^2 / t: what the reference's unit-norm assertion inspects) and the row
    statistics; for D <= 256 the 2n x 2n matrix itself exists only tile-wise inside the kernels."""

    @staticmethod
    def forward(ctx, P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float, exclude_pos: bool = False):
        ops.require_gpu(P)
        P = P.float().contiguous()
        ctx.excl = bool(exclude_pos)
        ctx.fused = ops.supcon_fused_ok(P) and not ctx.excl
        if ctx.excl:  # exclude_other_pos=True (contrastive.py:87-91): on the materialised matrix
            loss, S, stats, tmp = ops.supcon_excl_fwd(P, labels, pos_mask, t)
            diag = S.diagonal().clone()
            ctx.save_for_backward(P, stats, S, tmp)
        elif ctx.fused:
            loss, diag, stats = ops.supcon_fwd_fused(P, labels, pos_mask, t)
            ctx.save_for_backward(P, stats)
        else:
            loss, S, stats = ops.supcon_fwd(P, labels, pos_mask, t)
            diag = S.diagonal().clone()
            ctx.save_for_backward(P, stats, S)
        ctx.labels, ctx.pos_mask, ctx.t = labels, pos_mask, t
        ctx.mark_non_differentiable(diag, stats)
        return loss, diag, stats

    @staticmethod
    def backward(ctx, g: Tensor, _gd, _gstats):
        gs = g.reshape(1).float().contiguous()
        if ctx.excl:
            P, stats, S, tmp = ctx.saved_tensors
            return ops.supcon_excl_bwd(P, ctx.labels, ctx.pos_mask, S, stats, tmp, gs, ctx.t), None, None, None, None
        if ctx.fused:
            P, stats = ctx.saved_tensors
            return ops.supcon_bwd_fused(P, ctx.labels, ctx.pos_mask, stats, gs, ctx.t), None, None, None, None
        P, stats, S = ctx.saved_tensors
        return ops.supcon_bwd(P, ctx.labels, ctx.pos_mask, S, stats, gs, ctx.t), None, None, None, None


class SelfPacedSupConFn(torch.autograd.Function):
    """SelfPacedSupConLoss (contrastyou/losses/contrastive.py:103-212) on P = cat(z1, z2), D <= 256 and D % 8 == 0: the
    fused SupCon tiles with a second forward pass for the self-paced weights.  Returns the loss, the self-paced ratio
    (both 0-dim device tensors), the diagonal of the similarity matrix and the row statistics (D_i, c_i, W_i, M); only
    the loss is differentiable -- the weights and the ratio are constants of the gradient, as in the reference."""

    @staticmethod
    def forward(ctx, P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float, gamma: float,
                soft: bool, correct_grad: bool):
        ops.require_gpu(P)
        P = P.float().contiguous()
        aux, diag, stats = ops.supcon_sp_fwd(P, labels, pos_mask, t, gamma, soft, correct_grad)
        ctx.save_for_backward(P, stats, aux)
        ctx.labels, ctx.pos_mask, ctx.t, ctx.gamma, ctx.soft = labels, pos_mask, t, gamma, soft
        loss, ratio = aux[0], aux[1]
        ctx.mark_non_differentiable(ratio, diag, stats)
        return loss, ratio, diag, stats

    @staticmethod
    def backward(ctx, g: Tensor, _gr, _gd, _gstats):
        P, stats, aux = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        dP = ops.supcon_sp_bwd(P, ctx.labels, ctx.pos_mask, stats, aux, gs, ctx.t, ctx.gamma, ctx.soft)
        return dP, None, None, None, None, None, None


class AffineFn(torch.autograd.Function):
    """Nearest-neighbour affine resampling (+gamma), the in-step augmentation of
    semi_seg/augment.py:297-311 with the geometry given explicitly as theta."""

    @staticmethod
    def forward(ctx, x: Tensor, theta: Tensor, gamma: Optional[Tensor]):
        ops.require_gpu(x, theta)
        ctx.save_for_backward(theta)
        ctx.has_gamma = gamma is not None
        return ops.affine_fwd(x, theta, gamma)

    @staticmethod
    def backward(ctx, g: Tensor):
        if ctx.has_gamma:
            raise RuntimeError("backward through the gamma (image-mode) transform is not defined: "
                               "the reference applies it to input images only")
        (theta,) = ctx.saved_tensors
        return ops.affine_bwd(g, theta), None, None


# ------------------------------------------------------------------------------------------------
# dense contrastive projector, point sampling, cluster heads, discrete MI, GroupNorm block
# ------------------------------------------------------------------------------------------------
class DenseProjHiddenFn(torch.autograd.Function):
    """mean over adaptive-pool bins of LeakyReLU(Conv1x1(x)) -> [bins, hid]: the fused front half of
    DenseProjectionHead (contrastyou/projectors/heads.py:31-41,99-123); the second 1x1 conv commutes
    with the average pool and is applied to the pooled rows."""

    @staticmethod
    def forward(ctx, x: Tensor, w1: Tensor, b1: Tensor, size, bins: Optional[Tensor]):
        ops.require_gpu(x, w1)
        x = ops.to_nhwc(x)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        w = w1.detach().reshape(w1.shape[0], -1).float().contiguous()
        b = b1.detach().float().contiguous()
        ctx.save_for_backward(x, w, b)
        ctx.size, ctx.bins = tuple(size), bins
        return ops.dense_proj_fwd(x, w, b, ctx.size, bins)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w, b = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dw, db = ops.dense_proj_bwd(x, w, b, ctx.size, ctx.bins, g.float().contiguous(), need_dx, need_dw)
        if dw is not None:
            dw = dw.view(dw.shape[0], dw.shape[1], 1, 1)
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None


class PixelMLPFn(torch.autograd.Function):
    """DenseProjectionHead without pooling (contrastyou/projectors/heads.py:99-123 with projectors/nn.py:16-23
    `Identical`): Conv1x1(C, hid) -> LeakyReLU(slope) -> Conv1x1(hid, out) [-> F.normalize over channels] on every
    pixel, or on the listed pixels only, in one launch (csrc/cy_pixel_mlp.hip; the hidden activations never reach
    memory).  x: an [N, C, H, W] map (read as NHWC) or rows [R, C]; idx: int32 device tensor of distinct rows
    (n*H*W + r*W + c) or None; w2 = b2 = None: the linear head.  -> f32 rows [M, out], M = len(idx) or R.
    The gradient of x is zero outside the listed rows."""

    @staticmethod
    def forward(ctx, x: Tensor, idx: Optional[Tensor], w1: Tensor, b1: Tensor, w2: Optional[Tensor],
                b2: Optional[Tensor], slope: float, normalize: bool):
        ops.require_gpu(x, w1, b1, w2, b2)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        ctx.map_shape = None
        if x.dim() == 4:
            x = ops.to_nhwc(x)
            ctx.map_shape = tuple(x.shape)
            rows = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])  # (a view: NHWC memory)
        else:
            rows = x if x.stride(1) == 1 else x.contiguous()
        w1f = w1.detach().reshape(w1.shape[0], -1).float().contiguous()
        b1f = b1.detach().float().contiguous()
        w2f = None if w2 is None else w2.detach().reshape(w2.shape[0], -1).float().contiguous()
        b2f = None if b2 is None else b2.detach().float().contiguous()
        y, inv = ops.pixel_mlp_fwd(rows, idx, w1f, b1f, w2f, b2f, slope, normalize)
        ctx.save_for_backward(rows, idx, w1f, b1f, w2f, y, inv)
        ctx.slope, ctx.normalize = float(slope), bool(normalize)
        ctx.shapes = (tuple(w1.shape), None if w2 is None else tuple(w2.shape))
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        rows, idx, w1f, b1f, w2f, y, inv = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_dw = need[2] or need[3] or (w2f is not None and (need[4] or need[5]))
        dx, dw1, db1, dw2, db2 = ops.pixel_mlp_bwd(rows, idx, w1f, b1f, w2f, y, inv, g.float().contiguous(), ctx.slope,
                                                   ctx.normalize, need[0], need_dw)
        if dx is not None and ctx.map_shape is not None:
            n, c, h, w = ctx.map_shape
            dx = dx.view(n, h, w, c).permute(0, 3, 1, 2)
        s1, s2 = ctx.shapes
        return (dx, None, dw1.view(s1) if need[2] else None, db1 if need[3] else None,
                dw2.view(s2) if (w2f is not None and need[4]) else None,
                db2 if (w2f is not None and need[5]) else None, None, None)


class AdaptiveAvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(size) on an NHWC map -> f32 rows [N*sh*sw, C]"""

    @staticmethod
    def forward(ctx, x: Tensor, size):
        ops.require_gpu(x)
        x = ops.to_nhwc(x)
        ctx.shape, ctx.dtype, ctx.size = tuple(x.shape), x.dtype, tuple(size)
        return ops.adaptive_avgpool_fwd(x, ctx.size)

    @staticmethod
    def backward(ctx, g: Tensor):
        return ops.adaptive_avgpool_bwd(g.float().contiguous(), ctx.shape, ctx.dtype, ctx.size), None


class AdaptiveMaxPoolFn(torch.autograd.Function):
    """nn.AdaptiveMaxPool2d(size) on an NHWC map -> f32 rows [N*sh*sw, C] (contrastyou/projectors/nn.py:16-23,
    pool_name="adaptive_max")"""

    @staticmethod
    def forward(ctx, x: Tensor, size):
        ops.require_gpu(x)
        x = ops.to_nhwc(x)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        ctx.shape, ctx.dtype, ctx.size = tuple(x.shape), x.dtype, tuple(size)
        out, arg = ops.adaptive_maxpool_fwd(x, ctx.size)
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (arg,) = ctx.saved_tensors
        return ops.adaptive_maxpool_bwd(g.float().contiguous(), arg, ctx.shape, ctx.dtype, ctx.size), None


class GatherRowsFn(torch.autograd.Function):
    """rows[idx] for distinct idx (the point sampling of semi_seg/hooks/infonce.py:31-46)"""

    @staticmethod
    def forward(ctx, src: Tensor, idx: Tensor):
        src = src.float().contiguous()
        ctx.save_for_backward(idx)
        ctx.rows = src.shape[0]
        return ops.gather_rows_fwd(src, idx)

    @staticmethod
    def backward(ctx, g: Tensor):
        (idx,) = ctx.saved_tensors
        return ops.gather_rows_bwd(g.float().contiguous(), idx, ctx.rows), None


class GroupSoftmaxFn(torch.autograd.Function):
    """[M, S*k] logits -> [S, M, k] probabilities, softmax(logits / T) inside each sub-head
    (SoftmaxWithT, contrastyou/projectors/nn.py:35-44)"""

    @staticmethod
    def forward(ctx, logits: Tensor, S: int, k: int, T: float):
        logits = logits.float().contiguous()
        probs = ops.group_softmax_fwd(logits, S, k, T)
        ctx.save_for_backward(probs)
        ctx.T = T
        return probs

    @staticmethod
    def backward(ctx, g: Tensor):
        (probs,) = ctx.saved_tensors
        return ops.group_softmax_bwd(probs, g.float().contiguous(), ctx.T), None, None, None


class ClusterHeadFn(torch.autograd.Function):
    """stacked 1x1 conv / linear (S*k <= 128 outputs) + per-sub-head softmax(./T) in one pass on the f32 MFMA:
    rows x [M, C] -> probs [S, M, k]; the logits never reach memory (csrc/cy_cluster_head.hip;
    contrastyou/projectors/heads.py:125-173, projectors/nn.py:35-44)"""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Optional[Tensor], S: int, k: int, T: float):
        ops.require_gpu(x, w)
        x = x.contiguous()
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        w2 = w.detach().reshape(S * k, -1).float().contiguous()
        probs = ops.cluster_head_fwd(x, w2, None if b is None else b.detach().float().contiguous(), S, k, T)
        ctx.save_for_backward(x, w2, probs)
        ctx.T, ctx.w_shape, ctx.has_bias = T, w.shape, b is not None
        return probs

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w2, probs = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dw = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dx, dw, db = ops.cluster_head_bwd(x, w2, probs, g.float().contiguous(), ctx.T, need_dx, need_dw)
        return (dx, dw.view(ctx.w_shape) if (dw is not None and ctx.needs_input_grad[1]) else None,
                db if (ctx.has_bias and ctx.needs_input_grad[2]) else None, None, None, None)


class IIDFn(torch.autograd.Function):
    """joint of two probability maps + information loss in one autograd node.
    x1, x2: f32 [N,H,W,k] contiguous (vectors: H=W=1).  mode 0/1: IIDSegmentationLoss with padding
    0 / >0; mode 2: IIDLoss (contrastyou/losses/discreteMI.py:90-170,201-261).
    Returns (loss, loss with lambda=1, normalised joint [T*T,k,k])."""

    @staticmethod
    def forward(ctx, x1: Tensor, x2: Tensor, mode: int, pad: int, symmetric: bool, lamda: float, eps: float):
        ops.require_gpu(x1, x2)
        N, H, W, k = x1.shape
        normalise = mode == 0
        J = ops.joint_fwd(x1, x2, N, H, W, k, pad, normalise)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out2, P, dJ = ops.iid_loss(J, mode, symmetric, lamda, eps, want_grad=need)
        ctx.save_for_backward(x1, x2, dJ)
        ctx.cfg = (N, H, W, k, pad, normalise)
        ctx.mark_non_differentiable(P)
        return out2[0], out2[1].detach(), P

    @staticmethod
    def backward(ctx, g: Tensor, _g1, _gP):
        x1, x2, dJ = ctx.saved_tensors
        N, H, W, k, pad, normalise = ctx.cfg
        gs = g.reshape(1).float().contiguous()
        d1, d2 = ops.joint_bwd(x1, x2, dJ, gs, N, H, W, k, pad, normalise, ctx.needs_input_grad[0],
                               ctx.needs_input_grad[1])
        return d1, d2, None, None, None, None, None


class IIDPatchFn(torch.autograd.Function):
    """patch-wise IIC (IIDSegmentationSmallPathLoss, contrastyou/losses/discreteMI.py:173-198) in one autograd node:
    the joints of all patches in one launch, one block per patch for the losses, their mean.
    x1, x2: f32 [N,H,W,k] contiguous.  Returns (loss, per-patch losses [P], final joints [P,T*T,k,k])."""

    @staticmethod
    def forward(ctx, x1: Tensor, x2: Tensor, pad: int, patch: int, lamda: float, eps: float):
        ops.require_gpu(x1, x2)
        normalise = pad == 0
        J = ops.joint_patch_fwd(x1, x2, pad, patch, normalise)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, losses, Pj, dJ = ops.iid_patch_loss(J, 0 if pad == 0 else 1, lamda, eps, want_grad=need)
        ctx.save_for_backward(x1, x2, dJ)
        ctx.cfg = (pad, patch, normalise)
        ctx.mark_non_differentiable(losses, Pj)
        return loss[0], losses, Pj

    @staticmethod
    def backward(ctx, g: Tensor, _gl, _gP):
        x1, x2, dJ = ctx.saved_tensors
        pad, patch, normalise = ctx.cfg
        gs = g.reshape(1).float().contiguous()
        d1, d2 = ops.joint_patch_bwd(x1, x2, dJ, gs, pad, patch, normalise, ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1])
        return d1, d2, None, None, None, None


class PUIFn(torch.autograd.Function):
    """PUILoss (contrastyou/losses/pica_loss.py:10-39) on f32 [N,K] contiguous rows: the numerator from cy_joint_fwd, the
    column norms and means from one column reduction, one finishing block; the gradient flows back through all three."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, lamda: float):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, dJ, coef = ops.pui_loss(x, y, lamda, want_grad=need)
        ctx.save_for_backward(x, y, dJ, coef)
        return out[0]

    @staticmethod
    def backward(ctx, g: Tensor):
        x, y, dJ, coef = ctx.saved_tensors
        dx, dy = ops.pui_loss_bwd(x, y, dJ, coef, g.reshape(1).float().contiguous(), ctx.needs_input_grad[0],
                                  ctx.needs_input_grad[1])
        return dx, dy, None


class PUISegFn(torch.autograd.Function):
    """PUISegLoss (contrastyou/losses/pica_loss.py:42-85) on f32 [N,H,W,k] contiguous maps: cy_joint_fwd, the streaming
    balance term over x1, one finishing block."""

    @staticmethod
    def forward(ctx, x1: Tensor, x2: Tensor, pad: int, lamda: float):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, dJ = ops.puiseg_loss(x1, x2, pad, lamda, want_grad=need)
        ctx.save_for_backward(x1, x2, dJ)
        ctx.cfg = (pad, lamda)
        return out[0]

    @staticmethod
    def backward(ctx, g: Tensor):
        x1, x2, dJ = ctx.saved_tensors
        pad, lamda = ctx.cfg
        d1, d2 = ops.puiseg_loss_bwd(x1, x2, dJ, g.reshape(1).float().contiguous(), pad, lamda,
                                     ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d1, d2, None, None


def _jsd_layout(t: Tensor):
    """-> (buffer, R, C, S, shape of the unreduced output, back): rows and NHWC maps are read as [R][C] (S = 1), every
    other map as contiguous NCHW with S positions per image; `back` maps a gradient buffer to the input's shape"""
    Cc = t.shape[1]
    if t.dim() == 2:
        b = t.contiguous()
        return b, b.shape[0], Cc, 1, (t.shape[0],), lambda gr: gr
    if ops.is_nhwc(t) and not t.is_contiguous():
        b = t.permute(0, 2, 3, 1)  # contiguous [N,H,W,C]
        return b, b.numel() // Cc, Cc, 1, (t.shape[0], *t.shape[2:]), lambda gr: gr.permute(0, 3, 1, 2)
    b = t.contiguous()
    S = b.numel() // (b.shape[0] * Cc)
    return b, b.shape[0] * S, Cc, S, (t.shape[0], *t.shape[2:]), lambda gr: gr


class JSDFn(torch.autograd.Function):
    """JSD_div (contrastyou/losses/kl.py:142-174): Entropy(mean of the maps) - mean of the Entropies, one fused pass over
    the maps each way.  apply(reduction, eps, *maps)"""

    @staticmethod
    def forward(ctx, reduction: str, eps: float, *maps: Tensor):
        ops.require_gpu(*maps)
        first, R, Cc, S, out_shape, back = _jsd_layout(maps[0])
        bufs = [first]
        for t in maps[1:]:  # the layout of the first map for all
            if S == 1 and t.dim() > 2:
                bufs.append(t.permute(0, 2, 3, 1).contiguous())
            else:
                bufs.append(t.contiguous())
        out = ops.jsd_fwd(bufs, R, Cc, S, reduction, eps)
        ctx.save_for_backward(*bufs)
        ctx.cfg = (R, Cc, S, reduction, eps, back)
        return out.view(out_shape) if reduction == "none" else out[0]

    @staticmethod
    def backward(ctx, g: Tensor):
        R, Cc, S, reduction, eps, back = ctx.cfg
        grads = ops.jsd_bwd(ctx.saved_tensors, g.reshape(-1).float().contiguous(), ctx.needs_input_grad[2:], R, Cc, S,
                            reduction, eps)
        return (None, None, *[None if gr is None else back(gr) for gr in grads])


class EntropyPriorFn(torch.autograd.Function):
    """EntropyPrior (contrastyou/losses/kl.py:63-78): log C - KL_div()(prior, x) on f32 [R,C] rows with a broadcast
    prior row (None: uniform), which is a constant."""

    @staticmethod
    def forward(ctx, x: Tensor, prior, eps: float):
        x = x.contiguous()
        out = ops.entropy_prior_fwd(x, prior, eps)
        ctx.save_for_backward(x, prior)
        ctx.eps = eps
        return out[0]

    @staticmethod
    def backward(ctx, g: Tensor):
        x, prior = ctx.saved_tensors
        return ops.entropy_prior_bwd(x, prior, g.reshape(1).float().contiguous(), ctx.eps), None, None


class JointFn(torch.autograd.Function):
    """the k x k joint of two probability maps, (1/npix) sum_p x1[p,:] x2[p,:]^T, as its own autograd node
    (compute_joint_2D_with_padding_zeros, contrastyou/losses/discreteMI.py:246-261, before symmetrisation):
    the pixel contraction on the HIP joint kernels, whatever follows on the k x k result in plain autograd.
    x1, x2: f32 [N,H,W,k] contiguous."""

    @staticmethod
    def forward(ctx, x1: Tensor, x2: Tensor):
        ops.require_gpu(x1, x2)
        N, H, W, k = x1.shape
        ctx.save_for_backward(x1, x2)
        return ops.joint_fwd(x1, x2, N, H, W, k, 0, True).view(k, k)

    @staticmethod
    def backward(ctx, g: Tensor):
        x1, x2 = ctx.saved_tensors
        N, H, W, k = x1.shape
        one = torch.ones(1, device=g.device, dtype=torch.float32)
        d1, d2 = ops.joint_bwd(x1, x2, g.float().contiguous().view(1, k, k), one, N, H, W, k, 0, True,
                               ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d1, d2


def _imsat_rows(x: Tensor) -> Tensor:
    """[R, K] rows or a [b, K, ...] map of any memory format -> its f32 rows [R, K], contiguous (a view where the
    channels already are innermost in memory)"""
    ops.require_gpu(x)
    if x.dim() == 4:
        return ops.to_nhwc(x.float()).permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    return x.float().movedim(1, -1).reshape(-1, x.shape[1]).contiguous()


def _imsat_grad(d: Tensor, like) -> Tensor:
    """rows [R, K] -> the (shape, dtype) of the input they are the gradient of"""
    shape, dtype = list(like[0]), like[1]
    return d.view(shape[:1] + shape[2:] + shape[1:2]).movedim(-1, 1).to(dtype)


def _grad_vector(*gs: Tensor) -> Tensor:
    """the upstream gradients of a function's scalars as one device vector (no host sync)"""
    return torch.stack([g.reshape(()).float() for g in gs])


class IMSATFn(torch.autograd.Function):
    """imsat_with_entropy(p) -> (marginal entropy, mean conditional entropy) of the probability rows of p, [R, K] or
    [b, K, H, W] in any memory format (contrastyou/losses/discreteMI.py:287-297); eps = 1e-8.  One read forward, one
    read and one write backward (csrc/cy_imsat.hip).

    `tangent`: for a p that is the output of a softmax.  The marginal's gradient c_k is the same in every row, and
    where the marginals are balanced the c_k are nearly equal; a softmax backward (dp - sum_j p_j dp_j) removes that
    common part again, by a subtraction that costs it the leading digits in f32.  With `tangent` the coefficients are
    handed on as c_k - sum_j m_j c_j: the same gradient on the simplex (a row-constant apart, which the softmax
    backward annihilates exactly), without the common part.  The result is then not dL/dp of an unconstrained p."""

    @staticmethod
    def forward(ctx, p: Tensor, tangent: bool = False):
        rows = _imsat_rows(p)
        out, coef, mean = ops.imsat_fwd(rows)
        ctx.save_for_backward(rows, coef, mean)
        ctx.like, ctx.tangent = (p.shape, p.dtype), tangent
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_marg: Tensor, g_cond: Tensor):
        rows, coef, mean = ctx.saved_tensors
        if ctx.tangent:
            coef = coef - (mean * coef).sum()
        return _imsat_grad(ops.imsat_bwd(rows, coef, _grad_vector(g_marg, g_cond)), ctx.like), None


class IMSATPairFn(torch.autograd.Function):
    """two views of the same shape -> (marg1, cond1, marg2, cond2, mse): the entropies of IMSATFn for each and
    nn.MSELoss()(x1, x2), each input read once (semi_seg/hooks/discretemi.py:148-167)"""

    @staticmethod
    def forward(ctx, x1: Tensor, x2: Tensor):
        assert x1.shape == x2.shape, (x1.shape, x2.shape)
        r1, r2 = _imsat_rows(x1), _imsat_rows(x2)
        out, coef, _ = ops.imsat_pair_fwd(r1, r2)
        ctx.save_for_backward(r1, r2, coef)
        ctx.like = ((x1.shape, x1.dtype), (x2.shape, x2.dtype))
        return tuple(out.unbind(0))

    @staticmethod
    def backward(ctx, *gs: Tensor):
        r1, r2, coef = ctx.saved_tensors
        d1, d2 = ops.imsat_pair_bwd(r1, r2, coef, _grad_vector(*gs))
        return (_imsat_grad(d1, ctx.like[0]) if ctx.needs_input_grad[0] else None,
                _imsat_grad(d2, ctx.like[1]) if ctx.needs_input_grad[1] else None)


class SoftmaxIMSATFn(torch.autograd.Function):
    """imsat_with_entropy(logits.softmax(1)) of an [N, K, H, W] logit map, K <= 16, without the probabilities in
    memory (semi_seg/hooks/midl.py:83-90); `softmax_imsat` is the entry for any K"""

    @staticmethod
    def forward(ctx, logits: Tensor):
        ops.require_gpu(logits)
        z = ops.to_nhwc(logits.float())
        out, coef, _ = ops.softmax_imsat_fwd(z)
        ctx.save_for_backward(z, coef)
        ctx.dtype = logits.dtype
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_marg: Tensor, g_cond: Tensor):
        z, coef = ctx.saved_tensors
        return ops.softmax_imsat_bwd(z, coef, _grad_vector(g_marg, g_cond)).to(ctx.dtype)


def softmax_imsat(logits: Tensor):
    """(marg, cond) of softmax(logits, 1): the fused kernels up to 16 classes; past them the row-softmax kernel
    followed by the probability-row kernels (the way KL_div composes past 16)"""
    n, k, h, w = logits.shape
    if k <= ops.IMSAT_LOGITS_KMAX:
        return SoftmaxIMSATFn.apply(logits)
    ops.require_gpu(logits)
    flat = ops.to_nhwc(logits.float()).permute(0, 2, 3, 1).reshape(n * h * w, k)
    return IMSATFn.apply(GroupSoftmaxFn.apply(flat, 1, k, 1.0)[0], True)


class SgemmFn(torch.autograd.Function):
    """alpha * A @ B^T on the exact f32 MFMA kernel, differentiable in both operands"""

    @staticmethod
    def forward(ctx, A: Tensor, B: Tensor, alpha: float):
        ops.require_gpu(A, B)
        A, B = A.float().contiguous(), B.float().contiguous()
        ctx.save_for_backward(A, B)
        ctx.alpha = alpha
        return ops.sgemm(A, B, alpha, True)

    @staticmethod
    def backward(ctx, g: Tensor):
        A, B = ctx.saved_tensors
        g = g.float().contiguous()
        dA = ops.sgemm(g, B, ctx.alpha, False) if ctx.needs_input_grad[0] else None
        dB = ops.sgemm(g.t().contiguous(), A, ctx.alpha, False) if ctx.needs_input_grad[1] else None
        return dA, dB, None


class GNSiLUFn(torch.autograd.Function):
    """GroupNorm(G, C)(y + bias) -> SiLU on a raw (bias-free) conv output (arch/unet2.py:208-224)"""

    @staticmethod
    def forward(ctx, y: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, groups: int, eps: float):
        y = ops.to_nhwc(y)
        b = None if bias is None else bias.detach().float().contiguous()
        gm, bt = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        out, mr = ops.gn_silu_fwd(y, b, gm, bt, groups, eps)
        ctx.save_for_backward(y, b, gm, bt, mr)
        ctx.groups = groups
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        y, b, gm, bt, mr = ctx.saved_tensors
        g = ops.to_nhwc(g if g.dtype == y.dtype else g.to(y.dtype))
        du, dg, dbt, dbias = ops.gn_silu_bwd(y, g, b, gm, bt, mr, ctx.groups)
        return du, dbias, dg, dbt, None, None


class GNSiLUModFn(torch.autograd.Function):
    """GroupNorm(G, C)(y + bias) * (scale + 1) + shift -> SiLU: `Block.forward(x, scale_shift)` of the reference's
    time-embedded ResnetBlock (arch/unet2.py:208-224,240-246); scale / shift are [N, C] (f32)"""

    @staticmethod
    def forward(ctx, y: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, scale: Tensor, shift: Tensor,
                groups: int, eps: float):
        y = ops.to_nhwc(y)
        b = None if bias is None else bias.detach().float().contiguous()
        gm, bt = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        ms, mt = scale.detach().float().contiguous(), shift.detach().float().contiguous()
        out, mr = ops.gn_silu_mod_fwd(y, b, gm, bt, ms, mt, groups, eps)
        ctx.save_for_backward(y, b, gm, bt, ms, mt, mr)
        ctx.groups = groups
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        y, b, gm, bt, ms, mt, mr = ctx.saved_tensors
        g = ops.to_nhwc(g if g.dtype == y.dtype else g.to(y.dtype))
        du, dg, dbt, dbias, dms, dmt = ops.gn_silu_mod_bwd(y, g, b, gm, bt, ms, mt, mr, ctx.groups)
        return du, dbias, dg, dbt, dms, dmt, None, None


class ActFn(torch.autograd.Function):
    """elementwise SiLU (kind 0) / exact GELU (kind 1) on a small f32 tensor (UNet2's time-embedding MLPs)"""

    @staticmethod
    def forward(ctx, x: Tensor, kind: int):
        x = x.float().contiguous()
        ctx.save_for_backward(x)
        ctx.kind = kind
        return ops.act_fwd(x, kind)

    @staticmethod
    def backward(ctx, g: Tensor):
        (x,) = ctx.saved_tensors
        return ops.act_bwd(x, g.float().contiguous(), ctx.kind), None


class Conv3x3Fn(torch.autograd.Function):
    """bias-free 3x3 convolution (stride 1, padding 1) on the implicit-GEMM kernels; NHWC in/out.
    Used by the GroupNorm block, whose conv bias is folded into the normalisation kernels."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor):
        ops.require_gpu(x, w)
        x = ops.to_nhwc(x)
        wf, wd = packed_weights(w, x.dtype)
        out, _ = ops.conv3x3_fwd(x, None, wf, w.shape[0], want_stats=False)
        ctx.save_for_backward(x, w)
        ctx.wd = wd
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w = ctx.saved_tensors
        g = ops.to_nhwc(g if g.dtype == x.dtype else g.to(x.dtype))
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx, _ = ops.conv3x3_fwd(g, None, ctx.wd, x.shape[1], want_stats=False)
        if ctx.needs_input_grad[1]:
            dw = ops.conv3x3_wgrad(x, None, g).to(w.dtype)
        return dx, dw


def bilinear_resize(x: Tensor, size) -> Tensor:
    """F.interpolate(x, size=size, mode="bilinear") (align_corners=False) for inputs that carry no
    gradient -- the reference resizes input images only (semi_seg/hooks/cc.py:132)"""
    if x.requires_grad:
        raise RuntimeError("bilinear_resize: the HIP kernel is forward-only (input images carry no gradient)")
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.float()
    return ops.bilinear_fwd(x, tuple(size))


class EntropyMapFn(torch.autograd.Function):
    """probabilities [n, K, H, W] -> min/max-normalised entropy map [n, 1, H, W] (Entropy(reduction="none") + norm,
    semi_seg/hooks/ccblock.py:278-285,303; `slicewise=False`: the batch-wide extrema of semi_seg/hooks/cc.py:136).
    The extrema are constants of the backward pass (min().detach())."""

    @staticmethod
    def forward(ctx, prob: Tensor, slicewise: bool):
        ops.require_gpu(prob)
        prob = ops.to_nhwc(prob.float())
        out, mm = ops.entropy_map_fwd(prob, slicewise)
        ctx.save_for_backward(prob, mm)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        prob, mm = ctx.saved_tensors
        return ops.entropy_map_bwd(prob, mm, g.float().contiguous()), None


class CCLossFn(torch.autograd.Function):
    """CCLoss(win=(k, k), eps)(y_true, y_pred) on two [n, 1, H, W] maps (contrastyou/losses/cross_correlation.py:22-74);
    the backward recomputes the window sums from the two maps (csrc/cy_cc.hip)"""

    @staticmethod
    def forward(ctx, y_true: Tensor, y_pred: Tensor, win: int, eps: float):
        ops.require_gpu(y_true, y_pred)
        I, J = y_true.float().contiguous(), y_pred.float().contiguous()
        ctx.save_for_backward(I, J)
        ctx.win, ctx.eps = win, eps
        return ops.ccloss_fwd(I, J, win, eps)

    @staticmethod
    def backward(ctx, g: Tensor):
        I, J = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        dI, dJ = ops.ccloss_bwd(I, J, gs, ctx.win, ctx.eps, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dI, dJ, None, None


def edge_map(image: Tensor, power: float, size=None) -> Tensor:
    """norm(diff(image)) ** power of semi_seg/hooks/ccblock.py:296-302 (no gradient: images carry none), the image
    first resized to `size` when it differs (F.interpolate(mode="bilinear"), ccblock.py:300)"""
    with torch.no_grad():
        if size is not None and tuple(image.shape[-2:]) != tuple(size):
            image = bilinear_resize(image.detach(), (int(size[0]), int(size[1])))
        return ops.cc_edge_map(image, power)


# --------------------------------------------------------------------------- adversarial baseline (csrc/cy_disc.hip)
def _rows(x: Tensor) -> Tensor:
    """[N, C, H, W] (any memory format) -> f32 [N, H, W, C] contiguous; no copy when the memory is NHWC f32 already"""
    x = x.detach()
    return ops.to_nhwc(x if x.dtype == torch.float32 else x.float()).permute(0, 2, 3, 1).contiguous()


def _aligned16(t: Tensor) -> Tensor:
    """f32, contiguous, 16-byte aligned (a parameter that is a view into a flat buffer need not be)"""
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class SoftmaxCatFn(torch.autograd.Function):
    """torch.cat([image, logits.softmax(1)], 1), or logits.softmax(1) alone for image None
    (semi_seg/epochers/comparable.py:150-153): one pass over the logits each way; the image carries no gradient"""

    @staticmethod
    def forward(ctx, image: Optional[Tensor], logits: Tensor):
        ops.require_gpu(image, logits)
        z = ops.to_nhwc(logits.detach().float())
        img = None if image is None else ops.to_nhwc(image.detach().float())
        if img is not None and (img.shape[0], *img.shape[2:]) != (z.shape[0], *z.shape[2:]):
            raise ValueError(f"image {tuple(img.shape)} and logits {tuple(z.shape)} differ in batch or size")
        ctx.save_for_backward(z)
        ctx.ci = 0 if img is None else img.shape[1]
        return ops.softmax_cat_fwd(img, z).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout: Tensor):
        z, = ctx.saved_tensors
        return None, ops.softmax_cat_bwd(z, _rows(dout), ctx.ci)


class BNLeakyReLUFn(torch.autograd.Function):
    """nn.LeakyReLU(slope)(nn.BatchNorm2d(C)(x)) on an NHWC f32 map.  training: batch statistics, and the running
    statistics / counter (when given) are updated in place by the statistics kernel; otherwise the running statistics
    normalise.  The backward recomputes the pre-activation from x."""

    @staticmethod
    def forward(ctx, x: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor],
                running_var: Optional[Tensor], num_batches_tracked: Optional[Tensor], training: bool, momentum: float,
                eps: float, slope: float):
        ops.require_gpu(x, gamma, beta)
        xr = _rows(x)
        N, H, W, Cc = xr.shape
        x2d = xr.view(N * H * W, Cc)
        g, b = _aligned16(gamma), _aligned16(beta)
        batch = training or running_mean is None
        if batch:
            track = training and running_mean is not None
            mean, var = ops.bn_rows_stats(x2d, running_mean if track else None, running_var if track else None,
                                          num_batches_tracked if track else None, momentum)
        else:
            mean, var = _aligned16(running_mean), _aligned16(running_var)
        y = ops.bn_lrelu_fwd(x2d, mean, var, g, b, eps, slope)
        ctx.save_for_backward(x2d, mean, var, g, b)
        ctx.cfg = (float(eps), float(slope), batch, (N, H, W, Cc))
        return y.view(N, H, W, Cc).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy: Tensor):
        x2d, mean, var, g, b = ctx.saved_tensors
        eps, slope, batch, (N, H, W, Cc) = ctx.cfg
        dy2d = _rows(dy).view(N * H * W, Cc)
        need = ctx.needs_input_grad
        # running statistics and no parameter gradient wanted: dx = gamma * invstd * dz needs no sums
        dx, dg, db = ops.bn_lrelu_bwd(x2d, dy2d, mean, var, g, b, eps, slope, batch, need[0],
                                      need_sums=batch or need[1] or need[2])
        if dx is not None:
            dx = dx.view(N, H, W, Cc).permute(0, 3, 1, 2)
        return (dx, dg if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None)


class LeakyReLUFn(torch.autograd.Function):
    """nn.LeakyReLU(slope) on an [N, C, H, W] map (kept NHWC f32); the backward works from the input"""

    @staticmethod
    def forward(ctx, x: Tensor, slope: float):
        ops.require_gpu(x)
        xr = _rows(x)  # (the gradient arrives NHWC as well: one layout both ways)
        ctx.save_for_backward(xr)
        ctx.slope = float(slope)
        return ops.leaky_relu_fwd(xr, slope).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy: Tensor):
        xr, = ctx.saved_tensors
        return ops.leaky_relu_bwd(xr, _rows(dy), ctx.slope).permute(0, 3, 1, 2), None


class SigmoidBCEFn(torch.autograd.Function):
    """nn.BCELoss()(torch.sigmoid(scores), torch.full_like(scores, label)), label 0 or 1, from the scores: softplus of
    -s / s, clamped at 100 as torch clamps the logarithm; never forms 1 - sigmoid(s)"""

    @staticmethod
    def forward(ctx, scores: Tensor, label: float):
        ops.require_gpu(scores)
        if label not in (0, 1, 0.0, 1.0):
            raise ValueError(f"label must be 0 or 1, given {label!r}")
        s = scores.detach().float().contiguous()
        ctx.save_for_backward(s)
        ctx.label, ctx.shape = float(label), scores.shape
        return ops.sigmoid_bce_fwd(s, label)

    @staticmethod
    def backward(ctx, g: Tensor):
        s, = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        return ops.sigmoid_bce_bwd(s, ctx.label, gs).view(ctx.shape), None
