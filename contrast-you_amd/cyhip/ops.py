"""Tensor-level wrappers over the C ABI (one Python function per kernel family).

torch is used for device memory (caching allocator), the current HIP stream and nothing
else: every function below enqueues hand-written gfx950 kernels from libcontrastyou_hip.so.
Activations are logical [N,C,H,W] tensors in channels_last memory (= NHWC).
"""
from __future__ import annotations

import contextlib
import os
import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import CY_BF16, CY_F16, CY_F32, CY_SRC_DIRECT, CY_SRC_POOL2, CY_SRC_UP2, ConvDesc  # noqa: F401

_DT = {torch.float32: CY_F32, torch.bfloat16: CY_BF16, torch.float16: CY_F16}
HALF_TYPES = (torch.bfloat16, torch.float16)

# bench.py instrumentation: when a list, every conv launch appends (family, algorithmic FLOPs,
# start event, end event); events are recorded on the launch stream (torch's current stream).
PROFILE = None


class TimingEvent:
    """HIP event for measuring only (hipEventDisableSystemFence): torch.cuda.Event creates default events, whose
    recording performs a system-scope release -- an L2 writeback + invalidate that, around a single launch, falls
    inside the measured interval and slows the following kernel.  Recorded on torch's current stream."""

    __slots__ = ("_h",)

    def __init__(self):
        h = C.c_void_p()
        _lib.call("cy_debug_event_create", C.byref(h))
        self._h = h

    def record(self):
        _lib.call("cy_debug_event_record", self._h, _stream())
        return self

    def elapsed_time(self, other: "TimingEvent") -> float:
        """milliseconds from this event to `other` (waits for `other`) -- torch.cuda.Event's signature"""
        us = C.c_float()
        _lib.call("cy_debug_event_elapsed_us", self._h, other._h, C.byref(us))
        return us.value * 1e-3

    def __del__(self):
        try:
            _lib.call("cy_debug_event_destroy", self._h)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def _prof_begin():
    if PROFILE is None:
        return None
    return TimingEvent().record()


def _prof_end(e0, kind: str, flops: float, nbytes: float = 0.0):
    if e0 is None:
        return
    PROFILE.append((kind, flops, e0, TimingEvent().record(), nbytes))


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}: the HIP path computes in float32, bfloat16 or float16") from None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """raw hipStream_t of torch's current stream on the current device"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class PinnedRing:
    """small ring of pinned host buffers for sync-free H2D copies of per-step parameters.

    A non-blocking copy reads its pinned buffer when the stream reaches it, and nothing in a step makes the host wait
    for the GPU: a host running more than a ring's worth of uploads ahead would overwrite a buffer whose copy has not
    run yet (another step's augmentation parameters then reach the kernels).  Each slot therefore carries an event
    recorded behind its copy, and the host waits on it before refilling the slot -- it blocks only when it is that
    far ahead, where the GPU has a ring's worth of work queued anyway."""

    def __init__(self, slots: int = 16):
        self._slots, self._bufs, self._i = slots, {}, 0

    def upload(self, host: Tensor, device) -> Tensor:
        key = (tuple(host.shape), host.dtype)
        ring = self._bufs.get(key)
        if ring is None:
            ring = self._bufs[key] = [[torch.empty(host.shape, dtype=host.dtype).pin_memory(), None]
                                      for _ in range(self._slots)]
        self._i = (self._i + 1) % self._slots
        slot = ring[self._i]
        buf, done = slot
        capturing = torch.cuda.is_current_stream_capturing()
        if done is not None and not capturing:
            done.synchronize()  # the copy that last read this buffer has run
        buf.copy_(host)
        out = buf.to(device, non_blocking=True)
        if out.is_cuda and not capturing:
            if done is None:
                done = slot[1] = torch.cuda.Event()
            done.record(torch.cuda.current_stream(out.device))
        return out


pinned = PinnedRing()


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_gpu(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "contrast-you_amd: the hot path only runs as hand-written HIP kernels on a GPU "
                f"(got a {t.device} tensor); there is no CPU fallback")


def is_nhwc(t: Tensor) -> bool:
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def to_nhwc(t: Tensor) -> Tensor:
    """Return t with NHWC memory (no copy when it already is)."""
    if is_nhwc(t):
        return t
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def empty_nhwc(N: int, Cc: int, H: int, W: int, dtype, device) -> Tensor:
    return torch.empty((N, H, W, Cc), dtype=dtype, device=device).permute(0, 3, 1, 2)


def _f32(n, device) -> Tensor:
    return torch.empty(n, dtype=torch.float32, device=device)


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------- conv3x3
def packed_dims(Cout: int, Cin: int) -> Tuple[int, int]:
    a, b = C.c_int(), C.c_int()
    _lib.call("cy_conv3x3_packed_dims", Cout, Cin, C.byref(a), C.byref(b))
    return a.value, b.value


def packed_elems(Cout: int, Cin: int, dtype: torch.dtype) -> int:
    """elements of a packed weight image: [9, co_pad, ci_pad], then (16-bit, Cout % 64 == 0, Cin % 16 == 0) the
    stage-contiguous image of the LDS-DMA kernel (csrc/cy_conv_flow.h)"""
    return int(_lib.load().cy_conv3x3_packed_elems(Cout, Cin, dtype_code(dtype)))


def pack_weights(w: Tensor, dtype: torch.dtype, want_dgrad: bool = True):
    """w: [Cout,Cin,3,3] f32 -> (wf, wd or None): flat packed images of `dtype` (forward GEMM / data-gradient
    GEMM), packed_elems(Cout, Cin) / packed_elems(Cin, Cout) elements."""
    require_gpu(w)
    Cout, Cin = w.shape[0], w.shape[1]
    w = w.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    wf = torch.empty(packed_elems(Cout, Cin, dtype), dtype=dtype, device=w.device)
    wd = None
    if want_dgrad:
        wd = torch.empty(packed_elems(Cin, Cout, dtype), dtype=dtype, device=w.device)
    _lib.call("cy_conv3x3_pack_weights", w.data_ptr(), wf.data_ptr(), _ptr(wd), Cout, Cin,
              dtype_code(dtype), _stream())
    return wf, wd


class _PackSet:
    """device table + arena layout for packing a fixed list of 3x3 weights in one launch"""

    def __init__(self, weights, dtype):
        items = (_lib.PackItem * len(weights))()
        self.views = []  # per weight: (offset, elements) of the forward and of the dgrad image
        off_f = off_d = first = 0
        for it, w in zip(items, weights):
            Cout, Cin = w.shape[0], w.shape[1]
            cop, cip = packed_dims(Cout, Cin)
            cip2, cop2 = packed_dims(Cin, Cout)
            nf, nd = packed_elems(Cout, Cin, dtype), packed_elems(Cin, Cout, dtype)
            it.w, it.off_f, it.off_d, it.first = w.data_ptr(), off_f, off_d, first
            it.Cout, it.Cin, it.co_pad, it.ci_pad, it.ci_pad2, it.co_pad2 = Cout, Cin, cop, cip, cip2, cop2
            it.off_ff = off_f + 9 * cop * cip if nf > 9 * cop * cip else -1
            it.off_fd = off_d + 9 * cip2 * cop2 if nd > 9 * cip2 * cop2 else -1
            self.views.append(((off_f, nf), (off_d, nd)))
            off_f += nf
            off_d += nd
            first += -(-max(cop, cop2) // 32) * -(-max(cip, cip2) // 32)  # 32 x 32 (co, ci) tiles
        self.n, self.size_f, self.size_d, self.total = len(weights), off_f, off_d, first
        raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
        self.table = raw.to(weights[0].device)


_pack_sets = {}


def pack_weights_batched(weights, dtype: torch.dtype):
    """[(wf, wd)] for a list of [Cout,Cin,3,3] f32 weights, packed by ONE kernel launch into two fresh
    arenas (the per-layer views alias them).  The layer table lives on the device and is built once per
    (weight storages, dtype)."""
    require_gpu(*weights)
    for w in weights:
        if w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError("pack_weights_batched wants contiguous f32 weights")
    if len(weights) > 64:
        raise ValueError("at most 64 layers per batched pack")
    key = (dtype, tuple(w.data_ptr() for w in weights), tuple(tuple(w.shape) for w in weights))
    ps = _pack_sets.get(key)
    if ps is None:
        if len(_pack_sets) > 8:
            _pack_sets.clear()
        ps = _pack_sets[key] = _PackSet(weights, dtype)
    dev = weights[0].device
    af = torch.empty(ps.size_f, dtype=dtype, device=dev)
    ad = torch.empty(ps.size_d, dtype=dtype, device=dev)
    _lib.call("cy_conv3x3_pack_weights_batched", ps.table.data_ptr(), ps.n, ps.total, af.data_ptr(),
              ad.data_ptr(), dtype_code(dtype), _stream())
    out = []
    for (of, nf), (od, nd) in ps.views:
        out.append((af[of:of + nf], ad[od:od + nd]))
    return out


_desc_cache = {}


class _Plan:
    """a conv descriptor with the plan numbers the library derives from it (queried once per shape:
    the host issue path is the step's critical resource)"""
    __slots__ = ("d", "ref", "npart", "fwd_ws", "wgrad_ws", "pair_ws", "stat_wgs", "dgrad_bn")

    def __init__(self, d: ConvDesc):
        self.d, self.ref = d, C.byref(d)
        self.npart = self.fwd_ws = self.wgrad_ws = self.stat_wgs = self.dgrad_bn = None
        self.pair_ws = {}  # images of the second segment -> workspace bytes of the paired weight gradient


def _desc(N, H, W, C1, C2, Cout, mode, prologue, dt, ld1, ld2, ldo, split_c=0, ldo2=0) -> _Plan:
    key = (N, H, W, C1, C2, Cout, mode, prologue, dt, ld1, ld2, ldo, split_c, ldo2)
    p = _desc_cache.get(key)
    if p is None:
        d = ConvDesc()
        d.N, d.H, d.W, d.C1, d.C2, d.Cout = N, H, W, C1, C2, Cout
        d.mode1, d.prologue, d.in_dtype, d.out_dtype = mode, prologue, dt, dt
        d.ld1, d.ld2, d.ldo, d.split_c, d.ldo2 = ld1, ld2, ldo, split_c, ldo2
        p = _desc_cache[key] = _Plan(d)
    return p


def _query(struct, name: str, *args, skip=(), check: bool = True) -> dict:
    """a host-side query whose last argument is a `struct` the library fills in: the fields it answers, by name.
    `check` False: for the queries that answer a refusal in the struct's `status` field, nothing is raised"""
    s = struct()
    if check:
        _lib.call(name, *args, C.byref(s))
    else:
        getattr(_lib.load(), name)(*args, C.byref(s))
    return {f: getattr(s, f) for f, _ in s._fields_ if f not in skip}


def _fields(struct) -> tuple:
    return tuple(f for f, _ in struct._fields_)


# cy_conv_plan.kernel
KERNEL_NAMES = {_lib.CY_CONV_KERNEL_IGEMM: "conv3x3_igemm_kernel", _lib.CY_CONV_KERNEL_PLANE: "conv3x3_plane_kernel",
                _lib.CY_CONV_KERNEL_STREAM: "conv3x3_stream_kernel", _lib.CY_CONV_KERNEL_FLOW: "conv3x3_flow_kernel"}


def conv3x3_plan(N, H, W, C1, C2, Cout, dtype: torch.dtype, mode: int = 0, prologue: bool = False,
                 split: Optional[int] = None) -> dict:
    """the launch plan of cy_conv3x3_fwd for this layer geometry (host-side query, no GPU needed); `split`: of the
    form that writes out[:, :split] and out[:, split:] as two tensors (the data gradient of a concat layer)"""
    if split:
        d = _desc(N, H, W, C1, C2, Cout, mode, 1 if prologue else 0, dtype_code(dtype), C1, C2, split, split, Cout - split)
    else:
        d = _desc(N, H, W, C1, C2, Cout, mode, 1 if prologue else 0, dtype_code(dtype), C1, C2, Cout)
    out = _query(_lib.ConvPlan, "cy_conv3x3_plan", d.ref)
    out["kernel"] = KERNEL_NAMES[out["kernel"]]
    out["ws_bytes"] = int(_lib.load().cy_conv3x3_fwd_ws_bytes(d.ref))  # (the split-K workspace: 0 when ksplit == 1)
    return out


def conv3x3_wgrad_plan(N, H, W, C1, C2, Cout, dtype: torch.dtype, mode: int = 0, prologue: bool = False,
                       n_b: int = 0) -> dict:
    """the launch plan of cy_conv3x3_wgrad (n_b > 0: of cy_conv3x3_wgrad_pair) for this layer geometry"""
    d = _desc(N, H, W, C1, C2, Cout, mode, 1 if prologue else 0, dtype_code(dtype), C1, C2, Cout)
    return _query(_lib.WgradPlan, "cy_conv3x3_wgrad_plan", d.ref, n_b)


def _out_hw(src1: Tensor, mode: int) -> Tuple[int, int]:
    H, W = src1.shape[2], src1.shape[3]
    if mode == CY_SRC_POOL2:
        if H % 2 or W % 2:
            raise ValueError(f"max-pool 2x2 needs even spatial dims, got {H}x{W}")
        return H // 2, W // 2
    if mode == CY_SRC_UP2:
        return H * 2, W * 2
    return H, W


def conv3x3_fwd(src1: Tensor, src2: Optional[Tensor], wf: Tensor, Cout: int, *, mode: int = 0,
                scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
                want_stats: bool = True, split: Optional[int] = None, fold: Optional["BnState"] = None,
                stats_acc: bool = False):
    """out = conv3x3(cat(src1', src2)).  Returns (out, partials|None) or, with `split`,
    ((out[:, :split], out[:, split:]), None) as two separate NHWC tensors.
    `fold`: the BN+ReLU coefficients of source 1 come from the previous layer's accumulator (instead of scale / shift).
    `stats_acc`: the statistics go into a new accumulator: the second return value is (acc, R) instead of partial rows."""
    require_gpu(src1, wf)
    N, C1 = src1.shape[0], src1.shape[1]
    C2 = 0 if src2 is None else src2.shape[1]
    H, W = _out_hw(src1, mode)
    dt = dtype_code(src1.dtype)
    dev = src1.device
    prologue = 1 if (scale is not None or fold is not None) else 0
    if split:
        out = empty_nhwc(N, split, H, W, src1.dtype, dev)
        out2 = empty_nhwc(N, Cout - split, H, W, src1.dtype, dev)
        d = _desc(N, H, W, C1, C2, Cout, mode, prologue, dt, C1, C2, split, split, Cout - split)
    else:
        out = empty_nhwc(N, Cout, H, W, src1.dtype, dev)
        out2 = None
        d = _desc(N, H, W, C1, C2, Cout, mode, prologue, dt, C1, C2, Cout)
    stats = acc = None
    if want_stats and stats_acc:
        if d.stat_wgs is None:
            d.stat_wgs = _lib.call("cy_conv3x3_stat_workgroups", d.ref)
        acc = bn_acc_new(Cout, d.stat_wgs, dev)
    elif want_stats:
        if d.npart is None:
            d.npart = _lib.call("cy_conv3x3_num_partials", d.ref)
        stats = _f32(d.npart * 2 * Cout, dev).view(d.npart, 2, Cout)
    if d.fwd_ws is None:
        d.fwd_ws = _lib.load().cy_conv3x3_fwd_ws_bytes(d.ref)
    nbytes = d.fwd_ws
    ws = _ws(nbytes, dev) if nbytes else None
    ev = _prof_begin()
    if fold is not None or acc is not None:
        _lib.call("cy_conv3x3_fwd_bn", d.ref, src1.data_ptr(), _ptr(src2), None if fold is None else fold.ref,
                  _ptr(scale), _ptr(shift), wf.data_ptr(), out.data_ptr(), _ptr(out2), None,
                  None if acc is None else acc.ref, _ptr(ws), nbytes, _stream())
        stats = acc
        if fold is not None:
            fold.done = True
    else:
        _lib.call("cy_conv3x3_fwd", d.ref, src1.data_ptr(), _ptr(src2), _ptr(scale), _ptr(shift),
                  wf.data_ptr(), out.data_ptr(), _ptr(out2), _ptr(stats), _ptr(ws), nbytes, _stream())
    if ev is not None:  # algorithmic bytes: every input and output element once, packed weights once
        esz = src1.element_size()
        nb = esz * (src1.numel() + (0 if src2 is None else src2.numel()) + N * H * W * Cout + 9 * (C1 + C2) * Cout)
        _prof_end(ev, "conv3x3_fwd_dgrad", 2.0 * N * H * W * 9 * (C1 + C2) * Cout, float(nb))
    if split:
        return (out, out2), None
    return out, stats


# ---- side stream for weight gradients ------------------------------------------------------------
# A layer's weight-gradient kernels do not feed the rest of the backward pass (only the optimizer
# reads them), and at the configured batch sizes neither they nor the data-gradient kernels fill
# 256 CUs on their own.  They are therefore enqueued on a second HIP stream and overlap with the
# main stream's data-gradient / BN-backward kernels; the optimizer joins the stream before it reads
# the gradients.  CY_ASYNC_WGRAD=0 keeps everything on one stream.

ASYNC_WGRAD = os.environ.get("CY_ASYNC_WGRAD", "1") != "0"
CAPTURING = False  # True while a HIP graph of the step is being captured (cyhip.graphed)
_side_streams = {}
_side_pending = set()


def side_stream(device, role: str = "wgrad") -> "torch.cuda.Stream":
    """the per-device auxiliary stream of a role: "wgrad" (weight gradients) or "pass2" (second
    network pass of a two-stage step)"""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    st = _side_streams.get((idx, role))
    if st is None:
        # "comm" waits on a word in memory (stream_wait_marks): a waiting packet stalls every stream that shares its
        # hardware queue, and streams of one priority are multiplexed onto a few queues -- a stream of another
        # priority cannot share one with the streams that compute
        st = _side_streams[(idx, role)] = torch.cuda.Stream(device=idx, priority=-1 if role == "comm" else 0)
    return st


def note_side_work(stream) -> None:
    """register work on an auxiliary stream that the end-of-backward / optimizer join must wait for
    (call BEFORE enqueueing it: from here on in-place updates of shared buffers are event-ordered)"""
    global _multi_stream_live
    _multi_stream_live = True
    _side_pending.add(stream)


class on_side_stream:
    """run the enclosed launches on the side stream, after everything already enqueued on the
    current stream; `reads` are tensors the side kernels read (kept alive for the allocator)"""

    def __init__(self, *reads: Optional[Tensor]):
        self.reads = [t for t in reads if t is not None]

    def __enter__(self):
        dev = self.reads[0].device
        self.side = side_stream(dev)
        self.side.wait_stream(torch.cuda.current_stream(dev))
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self.side

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        if not CAPTURING:  # inside a graph capture lifetimes are the graph's; record_stream is not capturable
            for t in self.reads:
                t.record_stream(self.side)
        _side_pending.add(self.side)
        # join when this backward pass ends: .grad is then safe to read on the main stream
        _arm_backward_join(otherwise=join_side_streams)
        return False


_join_queued = False


def _arm_backward_join(otherwise=None) -> bool:
    """make sure `_join_after_backward` runs when the backward pass that is executing ends: True if it will.  When no
    backward pass is executing, `otherwise()` runs now instead (None: nothing does)."""
    global _join_queued
    if not _join_queued:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_join_after_backward)
            _join_queued = True
        except RuntimeError:  # not inside a backward pass
            if otherwise is not None:
                otherwise()
    return _join_queued


def ensure_backward_join() -> None:
    """called by backward nodes: if auxiliary streams carry work of this step (second-pass stream,
    weight-gradient stream) or work has been deferred to the end of the backward pass, make sure the
    deferred work is issued and the streams are joined when the backward pass ends"""
    if _side_pending or _at_backward_end or _wg_batches:
        _arm_backward_join()


_at_backward_end = []  # callables to run once when the current backward pass ends (before the joins)


def at_backward_end(fn) -> None:
    """run `fn()` when the backward pass that is executing ends (immediately if none is)"""
    if fn not in _at_backward_end:
        _at_backward_end.append(fn)
    _arm_backward_join(otherwise=_join_after_backward)


_in_join = False  # _join_after_backward is running (deferred work it issues is flushed by it)


def _join_after_backward() -> None:
    global _join_queued, _in_join
    _join_queued = False
    _in_join = True
    try:
        while _at_backward_end:
            _at_backward_end.pop(0)()
        join_side_streams()
        for idx in list(_wg_batches):  # the deferred slab sums, on the home stream after the join
            flush_wgrad_reduce(idx, onto=_home_stream.get(idx), final=True)
    finally:
        _in_join = False


_home_stream = {}  # device index -> the stream the step itself runs on


def note_home_stream(device) -> None:
    """remember the stream the network is driven from (called by the forward pass); the joins below
    target it explicitly because autograd's end-of-backward callbacks may run on a thread whose
    current stream is the legacy default stream"""
    cur = torch.cuda.current_stream(device)
    if cur not in _side_streams.values():
        _home_stream[cur.device.index] = cur


def join_side_streams(onto: Optional["torch.cuda.Stream"] = None) -> None:
    """make `onto` (default: the home stream of the device) wait for all side-stream work enqueued so far"""
    while _side_pending:
        st = _side_pending.pop()
        tgt = onto if onto is not None else _home_stream.get(st.device.index)
        if tgt is None:
            tgt = torch.cuda.current_stream(st.device)
        tgt.wait_stream(st)


# ---- "these gradients are final" marks for the data-parallel optimizer ----------------------------------------------
# The backward pass finishes the decoder's and the deep encoder blocks' gradients (85 % of the parameters) long before
# it ends.  A block whose backward has run for the LAST time in a step leaves a mark; FusedRAdam starts the all-reduce
# of the buckets whose parameters are all marked on a communication stream that waits for those marks only, while the
# rest of the backward pass -- eager, or a replayed HIP graph -- still runs.
# A mark must be visible from OUTSIDE a captured graph.  (CUDA's answer, an external event-record node, is refused by
# this runtime: hipEventRecordWithFlags(hipEventRecordExternal) returns hipErrorInvalidValue under capture.)  So a mark
# is a word in device memory: every step has a serial number, kept in a device scalar the host refreshes before the
# step's first pass; the mark is a tiny copy "flag[tag] <- serial" on a helper stream that waits for every stream
# carrying work of the step (an ordinary kernel + fork / join, capturable); the consumer stream waits until
# flag[tag] >= serial (hipStreamWaitValue32).
# OFF unless CY_DP_EARLY=1: correct in the two-rank rehearsals (tests/test_gpu_distributed.py), but in one process on a
# one-rank RCCL group (tools/dp_single_rank.py) the early start costs 0.24 ms of step time -- about what it could
# hide at N = 8.  Not something to switch on without a multi-GPU measurement.
# CY_DP_EARLY: "0" / "1" force it; unset = the rule of `dp_early_rule` (applied by FusedRAdam when its flat buffers are
# built, i.e. before any step is captured).
DP_EARLY = os.environ.get("CY_DP_EARLY", "0") == "1"
DP_EARLY_FORCED = os.environ.get("CY_DP_EARLY") in ("0", "1")


def dp_early_rule(grad_bytes: int, world: int) -> bool:
    """Start gradient buckets inside the backward pass only where the all-reduce they would otherwise expose behind it
    is worth more than the early start costs.  Measured cost of the early start on a one-rank RCCL group: 0.24 ms per
    step (tools/dp_single_rank.py).  Exposed time of the late order, estimated: a ring all-reduce
    moves 2 (w - 1) / w of the bytes per GPU; RCCL's multi-ring schedule over the seven xGMI links of a node reaches
    ~400 GB/s per GPU for tens of MB, plus ~2 x 30 us of collective latency.  On iff that estimate exceeds 0.3 ms:
    the 34.5 MB of U-Net gradients at 8 ranks give 0.21 ms -> off; models from ~55 MB of gradients up switch it on."""
    if world <= 1:
        return False
    exposed = 2.0 * (world - 1) / world * grad_bytes / 400e9 + 60e-6
    return exposed > 0.3e-3


marks_wanted = False   # set by a data-parallel FusedRAdam
MARK_TAGS = ("decoder", "conv5", "conv4")
_step_id = {}          # device index -> [int32 device scalar, host value]
_mark_flags = {}       # (device index, tag) -> int32 device scalar
_ready_marks = {}      # tag -> flag tensor, for the marks left in the current step


def _dev_index(device) -> int:
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def begin_step_marks(device) -> None:
    """a new step (forward + backward) begins on `device`: bump its serial.  Outside graph capture only."""
    if not (marks_wanted and DP_EARLY) or CAPTURING:
        return
    idx = _dev_index(device)
    rec = _step_id.get(idx)
    if rec is None:
        rec = _step_id[idx] = [torch.zeros(1, dtype=torch.int32, device=f"cuda:{idx}"), 0]
        for tag in MARK_TAGS:
            _mark_flags[(idx, tag)] = torch.zeros(1, dtype=torch.int32, device=f"cuda:{idx}")
    rec[1] += 1
    rec[0].fill_(rec[1])
    _ready_marks.clear()


def grad_ready_mark(tag: str, device) -> None:
    if not (marks_wanted and DP_EARLY) or tag not in MARK_TAGS:
        return
    idx = _dev_index(device)
    rec = _step_id.get(idx)
    if rec is None:
        return
    flag = _mark_flags[(idx, tag)]
    cur = torch.cuda.current_stream(idx)
    flush_wgrad_reduce(idx, onto=cur)  # (the deferred slab sums are part of the gradients the mark declares final)
    if torch.cuda.is_current_stream_capturing():
        # Inside the captured step the weight gradients stay on their pass's stream, and this stream has already
        # waited for whatever the other pass contributes to the block's parameters (the parked operands' events of the
        # paired weight gradients, recorded after that pass's BatchNorm finalize; the `ordered` accumulations): the
        # mark is one 4-byte copy in this stream's own order.  (Forked onto a helper stream it cost 0.35 ms of graph
        # time per mark -- cross-stream edges are expensive in a replayed graph.)
        flag.copy_(rec[0])
        _ready_marks[tag] = flag
        return
    helper = side_stream(idx, "mark")
    streams = {cur, _home_stream.get(idx, cur)} | {st for (d, role), st in _side_streams.items()
                                                   if d == idx and role not in ("mark", "comm")}
    for st in streams:  # (eager mode only: the capturing case returned above)
        ev = torch.cuda.Event()
        ev.record(st)
        helper.wait_event(ev)
    with torch.cuda.stream(helper):
        flag.copy_(rec[0])
    note_side_work(helper)  # joined when the backward pass ends (inside the capture, if there is one)
    ensure_backward_join()
    _ready_marks[tag] = flag


def take_ready_marks() -> dict:
    """the marks of the step (tag -> flag), handing them over: the next step starts without any"""
    m = dict(_ready_marks)
    _ready_marks.clear()
    return m


def set_ready_marks(marks: dict) -> None:
    """a replayed backward graph leaves the marks of its capture"""
    _ready_marks.clear()
    _ready_marks.update(marks)


def clear_ready_marks() -> None:
    _ready_marks.clear()


def stream_wait_marks(stream, flags, device) -> None:
    """`stream` waits until every flag carries the serial of the current step"""
    serial = _step_id[_dev_index(device)][1]
    for flag in flags:
        _lib.call("cy_stream_wait_value", stream.cuda_stream, flag.data_ptr(), serial)


# ---- cross-stream ordering of read-modify-write kernels -----------------------------------------
# With the two network passes of a step on two streams (SemiSupervisedEpocher two-stage forward) the
# kernels that update a shared buffer in place -- BN running statistics, accumulated BN parameter
# gradients, batch counters -- must keep the reference's order: every such launch waits for the last
# launch on the same buffer (if that was on another stream) and leaves an event behind.  The order is
# the host's enqueue order, so results stay deterministic.
TWO_STREAM = os.environ.get("CY_TWO_STREAM", "1") != "0"
_order_events = {}
_multi_stream_live = False  # set by the first fork onto a "pass2" stream; single-stream runs pay nothing


class ordered:
    """`with ordered(key):` -- serialise in-place updates of the buffer identified by `key` across streams"""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        if _multi_stream_live:
            rec = _order_events.get(self.key)
            if rec is not None:
                cur = torch.cuda.current_stream()
                # an event recorded outside a graph capture cannot be waited on inside one, nor one of
                # another capture; captures are fenced by full stream synchronisation, so skipping is safe
                if rec[1] != cur and rec[2] == _capture_id(cur):
                    cur.wait_event(rec[0])
        return self

    def __exit__(self, *exc):
        if _multi_stream_live:
            rec = _order_events.get(self.key)
            cur = torch.cuda.current_stream()
            cap = _capture_id(cur)
            ev = rec[0] if (rec is not None and rec[2] == cap) else torch.cuda.Event()
            ev.record(cur)
            _order_events[self.key] = (ev, cur, cap)
        return False


def _capture_id(stream) -> int:
    """0 outside HIP-graph capture, else the id of the capture `stream` belongs to"""
    if not torch.cuda.is_current_stream_capturing():
        return 0
    return int(_lib.load().cy_stream_capture_id(stream.cuda_stream))


def grad_sink(p: Tensor) -> Optional[Tensor]:
    """p.grad when the kernels can accumulate straight into it (f32, contiguous, on the GPU)"""
    if p is None or not p.is_leaf:
        return None
    g = p.grad
    if g is not None and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous():
        p.__dict__["_cy_touched"] = True  # read by FusedRAdam: this parameter received a gradient
        return g
    return None


def wgrad_reduce_entry(N, H, W, C1, C2, Cout, dtype: torch.dtype, mode: int = 0, prologue: bool = False,
                       n_b: int = 0) -> dict:
    """the slab-sum entry cy_conv3x3_wgrad (n_b > 0: _pair) makes for this layer geometry (host-side query)"""
    d = _desc(N, H, W, C1, C2, Cout, mode, 1 if prologue else 0, dtype_code(dtype), C1, C2, Cout)
    return _query(_lib.WgradReduceEntry, "cy_conv3x3_wgrad_reduce_entry", d.ref, n_b, skip=("ws", "dw"))


def first_wgrad_reduce_entry(N, Cin, H, W, Cout, dtype: torch.dtype) -> dict:
    """the partial-sum entry of cy_conv3x3_first_wgrad for these sizes (host-side query)"""
    return _query(_lib.WgradReduceEntry, "cy_conv3x3_first_wgrad_reduce_entry", N, Cin, H, W, Cout, dtype_code(dtype),
                  skip=("ws", "dw"))


# ---- deferred slab sums of the weight gradients ---------------------------------------------------------------------
# A weight gradient is an MFMA launch that writes f32 partial sums (slabs) and a reduce launch that adds them into dW.
# Only the optimizer (or an early data-parallel bucket) reads a live .grad, so for the gradients that go into one the
# reduce launches are collected and issued as ONE batched launch (cy_wgrad_reduce_batched): when the backward pass
# ends (home stream, after the side-stream join), before a "gradients final" mark, and when the table is full.  Every
# dW keeps the summation tree of its own reduce launch, so the results are bit-identical.  The slabs of a backward
# pass live in one arena (all at once: the cost of the deferral).
DEFER_WGRAD_REDUCE = True
# also flush (on the stream of the layer that crosses it) once this many slab bytes are pending: groups that the last
# level cache holds; None = only at the points above (the measured choice)
WGRAD_FLUSH_BYTES: Optional[int] = None


class SlabArena:
    """device memory for the slabs of one backward pass, sized by what earlier passes used; an allocation that does
    not fit gets a tensor of its own.  Released when the backward pass ends, after the batched reduce is enqueued."""
    high_water = 0

    def __init__(self, device):
        self.used = 0
        self.device = device
        self.bufs = []  # (tensor, stream it was allocated on): the arena first, then what did not fit
        n = SlabArena.high_water
        self.size = n
        if n:
            self.bufs.append((_ws(n, device), torch.cuda.current_stream(device)))

    def alloc(self, nbytes: int) -> int:
        a = self.used
        self.used += (int(nbytes) + 255) & ~255
        SlabArena.high_water = max(SlabArena.high_water, self.used)
        if self.used <= self.size:
            return self.bufs[0][0].data_ptr() + a
        t = _ws(nbytes, self.device)
        self.bufs.append((t, torch.cuda.current_stream(self.device)))
        return t.data_ptr()

    def release(self, last: "torch.cuda.Stream") -> None:
        """the last reader of the slabs is `last`: outside a capture the allocator must not hand the memory out again
        on the allocating stream before `last` has run (inside one the memory is the graph's)"""
        if not (CAPTURING or _lib.load().cy_stream_capture_id(last.cuda_stream)):
            for t, st in self.bufs:
                if st != last:
                    t.record_stream(last)
        self.bufs = []


class _WgradBatch:
    __slots__ = ("entries", "streams", "arena")

    def __init__(self, device):
        self.entries = []   # WgradReduceEntry, in issue order
        self.streams = set()  # streams that wrote slabs (or ran an earlier flush) in this backward pass
        self.arena = SlabArena(device)


_wg_batches = {}  # device index -> _WgradBatch of the backward pass that is executing


def _wg_batch(device) -> _WgradBatch:
    idx = _dev_index(device)
    b = _wg_batches.get(idx)
    if b is None:
        b = _wg_batches[idx] = _WgradBatch(torch.device("cuda", idx))
    return b


def _wg_defer(device, entry) -> None:
    """file a reduce entry whose MFMA launch was just enqueued on the current stream"""
    b = _wg_batch(device)
    b.entries.append(entry)
    b.streams.add(torch.cuda.current_stream(device))
    # the slab sums run when the backward pass ends; outside a backward pass nothing else comes: this one runs now
    if not _in_join and not _arm_backward_join(otherwise=lambda: flush_wgrad_reduce(device, final=True)):
        return
    if len(b.entries) >= _lib.CY_WGRAD_REDUCE_MAX or (
            WGRAD_FLUSH_BYTES is not None and sum(_slab_bytes(e) for e in b.entries) >= WGRAD_FLUSH_BYTES):
        flush_wgrad_reduce(device)


def _slab_bytes(e) -> int:
    return 4 * e.S * 9 * (e.co_pad * e.ci_pad if e.kind == _lib.CY_WGRAD_REDUCE_CONV else e.Cout * e.Cin)


def flush_wgrad_reduce(device=None, onto: Optional["torch.cuda.Stream"] = None, final: bool = False) -> None:
    """issue the deferred slab sums of `device` (all devices if None) as one batched launch on `onto` (default: the
    current stream; the home stream at the end of the backward pass), after every stream that wrote their slabs.
    `final`: the backward pass ends, the slab arena is released."""
    idxs = [_dev_index(device)] if device is not None else list(_wg_batches)
    for idx in idxs:
        b = _wg_batches.get(idx)
        if b is None:
            continue
        tgt = onto if onto is not None else torch.cuda.current_stream(idx)
        if b.entries:
            for st in b.streams:
                if st != tgt:
                    tgt.wait_stream(st)
            n = len(b.entries)
            arr = (_lib.WgradReduceEntry * n)(*b.entries)
            with torch.cuda.stream(tgt):
                ev = _prof_begin()
                _lib.call("cy_wgrad_reduce_batched", arr, n, _stream())
                if ev is not None:  # slabs read once, dW read (accumulate) and written
                    nb = sum(_slab_bytes(e) + 4.0 * (1 + e.accumulate) * 9 * e.Cout * e.Cin for e in b.entries)
                    _prof_end(ev, "wgrad_reduce", 0.0, nb)
            b.entries = []
            b.streams = {tgt}
            if tgt != _home_stream.get(idx):
                _side_pending.add(tgt)  # (joined when the backward pass ends)
        if final:
            b.arena.release(tgt)
            del _wg_batches[idx]


def conv3x3_wgrad(src1: Tensor, src2: Optional[Tensor], dy: Tensor, *, mode: int = 0,
                  scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
                  out: Optional[Tensor] = None, defer: bool = False) -> Tensor:
    """dw [Cout,Cin,3,3] f32; with `out` the result is ADDED into out (gradient accumulation).  `defer` (with `out`,
    a live .grad): the slab sum joins the batched launch of the backward pass (DEFER_WGRAD_REDUCE)."""
    require_gpu(src1, dy)
    N, C1 = src1.shape[0], src1.shape[1]
    C2 = 0 if src2 is None else src2.shape[1]
    Cout, H, W = dy.shape[1], dy.shape[2], dy.shape[3]
    dt = dtype_code(src1.dtype)
    d = _desc(N, H, W, C1, C2, Cout, mode, 1 if scale is not None else 0, dt, C1, C2, Cout)
    if d.wgrad_ws is None:
        d.wgrad_ws = _lib.load().cy_conv3x3_wgrad_ws_bytes(d.ref)
    nbytes = d.wgrad_ws
    defer = defer and out is not None and DEFER_WGRAD_REDUCE
    if defer:
        ev = _prof_begin()
        e = _lib.WgradReduceEntry()
        ws_ptr = _wg_batch(src1.device).arena.alloc(nbytes)
        _lib.call("cy_conv3x3_wgrad_deferred", d.ref, src1.data_ptr(), _ptr(src2), _ptr(scale), _ptr(shift),
                  dy.data_ptr(), out.data_ptr(), 1, ws_ptr, nbytes, C.byref(e), _stream())
        if ev is not None:
            esz = src1.element_size()
            nb = esz * (src1.numel() + (0 if src2 is None else src2.numel()) + dy.numel()) + 4 * 9 * (C1 + C2) * Cout
            _prof_end(ev, "conv3x3_wgrad", 2.0 * N * H * W * 9 * (C1 + C2) * Cout, float(nb))
        _wg_defer(src1.device, e)
        return out
    ws = _ws(nbytes, src1.device)
    dw = out if out is not None else torch.empty((Cout, C1 + C2, 3, 3), dtype=torch.float32, device=src1.device)
    ev = _prof_begin()
    # accumulation into a live .grad is a read-modify-write: the two passes of a step may reach the
    # same weight from different streams
    with (ordered(("conv_grad", out.data_ptr())) if out is not None else contextlib.nullcontext()):
        _lib.call("cy_conv3x3_wgrad", d.ref, src1.data_ptr(), _ptr(src2), _ptr(scale), _ptr(shift),
                  dy.data_ptr(), dw.data_ptr(), 0 if out is None else 1, ws.data_ptr(), nbytes, _stream())
    if ev is not None:
        esz = src1.element_size()
        nb = esz * (src1.numel() + (0 if src2 is None else src2.numel()) + dy.numel()) + 4 * 9 * (C1 + C2) * Cout
        _prof_end(ev, "conv3x3_wgrad", 2.0 * N * H * W * 9 * (C1 + C2) * Cout, float(nb))
    return dw


def conv3x3_wgrad_pair(src1: Tensor, src2: Optional[Tensor], dy: Tensor, scale: Optional[Tensor],
                       shift: Optional[Tensor], src1_b: Tensor, src2_b: Optional[Tensor], dy_b: Tensor,
                       scale_b: Optional[Tensor], shift_b: Optional[Tensor], *, mode: int, out: Tensor,
                       defer: bool = False) -> Tensor:
    """out += dw(segment a) + dw(segment b): the same layer on two batches (e.g. the two passes of a
    two-stage step) in ONE launch.  bf16 tensors of equal geometry per image.  `defer`: see conv3x3_wgrad."""
    require_gpu(src1, dy, src1_b, dy_b)
    N, C1 = src1.shape[0], src1.shape[1]
    C2 = 0 if src2 is None else src2.shape[1]
    Cout, H, W = dy.shape[1], dy.shape[2], dy.shape[3]
    if tuple(src1_b.shape[1:]) != tuple(src1.shape[1:]) or tuple(dy_b.shape[1:]) != tuple(dy.shape[1:]) \
            or src1_b.dtype != src1.dtype or (src2 is None) != (src2_b is None) or (scale is None) != (scale_b is None):
        raise ValueError("conv3x3_wgrad_pair: the two segments must be the same layer")
    d = _desc(N, H, W, C1, C2, Cout, mode, 1 if scale is not None else 0, dtype_code(src1.dtype), C1, C2, Cout)
    nb = src1_b.shape[0]
    nbytes = d.pair_ws.get(nb)
    if nbytes is None:
        nbytes = d.pair_ws[nb] = _lib.load().cy_conv3x3_wgrad_pair_ws_bytes(d.ref, nb)
    ev = _prof_begin()
    if defer and DEFER_WGRAD_REDUCE:
        e = _lib.WgradReduceEntry()
        _lib.call("cy_conv3x3_wgrad_pair_deferred", d.ref, src1.data_ptr(), _ptr(src2), _ptr(scale), _ptr(shift),
                  dy.data_ptr(), nb, src1_b.data_ptr(), _ptr(src2_b), _ptr(scale_b), _ptr(shift_b),
                  dy_b.data_ptr(), out.data_ptr(), 1, _wg_batch(src1.device).arena.alloc(nbytes), nbytes, C.byref(e),
                  _stream())
    else:
        e = None
        ws = _ws(nbytes, src1.device)
        with ordered(("conv_grad", out.data_ptr())):
            _lib.call("cy_conv3x3_wgrad_pair", d.ref, src1.data_ptr(), _ptr(src2), _ptr(scale), _ptr(shift),
                      dy.data_ptr(), nb, src1_b.data_ptr(), _ptr(src2_b), _ptr(scale_b), _ptr(shift_b),
                      dy_b.data_ptr(), out.data_ptr(), 1, ws.data_ptr(), nbytes, _stream())
    if ev is not None:
        esz = src1.element_size()
        nbts = esz * sum(t.numel() for t in (src1, src2, dy, src1_b, src2_b, dy_b) if t is not None) \
            + 4 * 9 * (C1 + C2) * Cout
        _prof_end(ev, "conv3x3_wgrad", 2.0 * (N + nb) * H * W * 9 * (C1 + C2) * Cout, float(nbts))
    if e is not None:
        _wg_defer(src1.device, e)
    return out


def conv_first_fwd(x: Tensor, w: Tensor, out_dtype: torch.dtype, want_stats: bool = True, stats_acc: bool = False):
    """x: f32 NCHW image [N,Cin<=4,H,W]; w: f32 [Cout,Cin,3,3]."""
    require_gpu(x, w)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    x = x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()
    w = w.detach().contiguous()
    out = empty_nhwc(N, Cout, H, W, out_dtype, x.device)
    stats = None
    if want_stats and stats_acc:
        npart = _lib.call("cy_conv3x3_first_num_partials", N, H, W, Cout)
        acc = bn_acc_new(Cout, npart, x.device)
        _lib.call("cy_conv3x3_first_fwd_acc", x.data_ptr(), w.data_ptr(), out.data_ptr(), acc.ref, N, Cin,
                  H, W, Cout, dtype_code(out_dtype), _stream())
        return out, acc
    if want_stats:
        npart = _lib.call("cy_conv3x3_first_num_partials", N, H, W, Cout)
        stats = _f32(npart * 2 * Cout, x.device).view(npart, 2, Cout)
    _lib.call("cy_conv3x3_first_fwd", x.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(stats), N, Cin,
              H, W, Cout, dtype_code(out_dtype), _stream())
    return out, stats


def conv_first_wgrad(x: Tensor, dy: Tensor, out: Optional[Tensor] = None, defer: bool = False) -> Tensor:
    """`defer`: see conv3x3_wgrad"""
    require_gpu(x, dy)
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    x = x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()
    nbytes = _lib.load().cy_conv3x3_first_wgrad_ws_bytes(N, Cin, H, W, Cout)
    if defer and out is not None and DEFER_WGRAD_REDUCE:
        e = _lib.WgradReduceEntry()
        _lib.call("cy_conv3x3_first_wgrad_deferred", x.data_ptr(), dy.data_ptr(), out.data_ptr(), 1, N, Cin, H, W,
                  Cout, dtype_code(dy.dtype), _wg_batch(x.device).arena.alloc(nbytes), nbytes, C.byref(e), _stream())
        _wg_defer(x.device, e)
        return out
    ws = _ws(nbytes, x.device)
    dw = out if out is not None else torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=x.device)
    with (ordered(("conv_grad", out.data_ptr())) if out is not None else contextlib.nullcontext()):
        _lib.call("cy_conv3x3_first_wgrad", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0 if out is None else 1,
                  N, Cin, H, W, Cout, dtype_code(dy.dtype), ws.data_ptr(), nbytes, _stream())
    return dw


# --------------------------------------------------------------------------- BN + ReLU
# BatchNorm sums without finalize launches (csrc/cy_bn_acc.h): producers add into a zeroed int64 accumulator, consumers
# derive the coefficients themselves.  CY_BN_ACC=0 keeps the partial rows + finalize launches of rounds 1-3 (A/B runs).
BN_ACC = os.environ.get("CY_BN_ACC", "1") != "0"


class BnArena:
    """zeroed int64 words for the accumulators of one network pass: ONE fill launch per pass instead of one per layer.
    The size follows what earlier passes used; an allocation that does not fit gets its own zeroed tensor."""
    high_water = 0

    def __init__(self, device):
        self.used = 0
        n = BnArena.high_water
        self.buf = torch.zeros(n, dtype=torch.int64, device=device) if n else None

    def alloc(self, words: int, device) -> Tensor:
        a = self.used
        self.used += (words + 15) & ~15  # (128-byte granules: no line is shared by two accumulators)
        if self.used > BnArena.high_water:
            BnArena.high_water = self.used
        if self.buf is not None and self.used <= self.buf.numel() and self.buf.device == torch.device(device):
            return self.buf[a:a + words]
        return torch.zeros(words, dtype=torch.int64, device=device)


_bn_arena: Optional[BnArena] = None


def bn_arena_begin(device) -> Optional[BnArena]:
    """called when a network pass begins; returns the previous arena (restored by `bn_arena_end`)"""
    global _bn_arena
    prev, _bn_arena = _bn_arena, (BnArena(device) if BN_ACC else None)
    return prev


def bn_arena_end(prev: Optional[BnArena]) -> None:
    global _bn_arena
    _bn_arena = prev


class BnAccBuf:
    """an accumulator [R][4][C] (+ R flags) and its ctypes view.

    The backward sums of a BatchNorm (sum dz, sum dz*xhat) may be added by whichever kernel writes the gradient dA of
    relu(bn(y)) while it has the values in registers: the max-pool backward of a block's output, the upsample backward
    or the data-gradient epilogue of the block that consumes it, the data-gradient epilogue inside the block.  The rule:
      * a producer adds into the accumulator only while it is `vacant`, and then records the tensor it wrote (`filled`);
      * the BatchNorm's backward uses the sums only if they were added for exactly the dA it holds (`holds`): autograd
        hands a single contribution through, but a sum of several consumers' gradients is another tensor, and the
        accumulator then holds a partial sum;
      * otherwise it runs the reduce launch into this accumulator if still vacant, else into a fresh one
        (`bn_acc_for_grad`)."""
    __slots__ = ("t", "R", "C", "s", "ref", "_filled_for")

    def __init__(self, t: Tensor, R: int, Cc: int):
        self.t, self.R, self.C = t, R, Cc
        self._filled_for = None
        self.s = _lib.BnAcc(t.data_ptr(), R, Cc)
        self.ref = C.byref(self.s)

    def vacant(self) -> bool:
        return self._filled_for is None

    def filled(self, da: Tensor) -> None:
        # (the tensor is kept alive: no address reuse, and `holds` also checks it was not written in place since)
        self._filled_for = da

    def holds(self, da: Optional[Tensor], y: Tensor) -> bool:
        made = self._filled_for
        return (made is not None and da is not None and da.data_ptr() == made.data_ptr()
                and da._version == made._version and da.shape == made.shape and da.dtype == y.dtype and is_nhwc(da))


def bn_acc_for_grad(acc: Optional[BnAccBuf], da: Optional[Tensor], y: Tensor) -> Tuple[Optional[BnAccBuf], bool]:
    """the consumer side of BnAccBuf's rule for the backward of relu(bn(y)) at `da`: (acc, True) if a producer added
    the sums of exactly `da`; else (accumulator for the reduce launch, False) -- `acc` while vacant, else None (the
    caller takes a fresh one)"""
    if acc is None or acc.vacant():
        return acc, False
    if acc.holds(da, y):
        return acc, True
    return None, False


def bn_acc_new(Cc: int, workgroups: int, device) -> BnAccBuf:
    R = _lib.call("cy_bn_acc_replicas", Cc, max(1, workgroups))
    words = R * 4 * Cc + R
    t = _bn_arena.alloc(words, device) if _bn_arena is not None else torch.zeros(words, dtype=torch.int64, device=device)
    return BnAccBuf(t, R, Cc)


class BnState:
    """one training-mode BatchNorm evaluation on an accumulator: what its consumer needs to derive relu(scale*y+shift)
    (cy_bn_fold) and where it leaves [scale, shift, mean, invstd, unbiased var] for the backward pass"""
    __slots__ = ("acc", "gamma", "beta", "count", "eps", "coef", "s", "ref", "done")

    def __init__(self, acc: BnAccBuf, gamma: Optional[Tensor], beta: Optional[Tensor], count: int, eps: float, device):
        self.acc, self.gamma, self.beta, self.count, self.eps = acc, gamma, beta, count, eps
        self.coef = _f32(5 * acc.C, device).view(5, acc.C)
        self.s = _lib.BnFold(acc.t.data_ptr(), acc.R, acc.C, _ptr(gamma), _ptr(beta), float(count), float(eps), 0,
                             self.coef.data_ptr())
        self.ref = C.byref(self.s)
        self.done = False  # a consumer has written `coef`


def bn_fold_coef(st: BnState) -> None:
    """accumulator -> st.coef as its own launch (when no folding consumer follows)"""
    _lib.call("cy_bn_fold_coef", st.ref, _stream())
    st.done = True


def bn_relu_apply_fold(y: Tensor, st: BnState, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    N, Cc, H, W = y.shape
    out_dtype = out_dtype or y.dtype
    out = empty_nhwc(N, Cc, H, W, out_dtype, y.device)
    _lib.call("cy_bn_relu_apply_fold", y.data_ptr(), st.ref, out.data_ptr(), N * H * W, dtype_code(y.dtype),
              dtype_code(out_dtype), _stream())
    st.done = True
    return out


def bn_relu_apply_pool_fold(y: Tensor, st: BnState) -> Tuple[Tensor, Tensor]:
    N, Cc, H2, W2 = y.shape
    if H2 % 2 or W2 % 2:
        raise ValueError(f"max-pool 2x2 needs even spatial dims, got {H2}x{W2}")
    out = empty_nhwc(N, Cc, H2, W2, y.dtype, y.device)
    pooled = empty_nhwc(N, Cc, H2 // 2, W2 // 2, y.dtype, y.device)
    dt = dtype_code(y.dtype)
    _lib.call("cy_bn_relu_apply_pool_fold", y.data_ptr(), st.ref, out.data_ptr(), pooled.data_ptr(), N, H2 // 2,
              W2 // 2, dt, dt, _stream())
    st.done = True
    return out, pooled


def bn_running_update(items) -> None:
    """items: [(coef [5, C], running_mean, running_var, momentum)] -- the running statistics of all of them in one
    launch per 32 layers, event-ordered against the other pass of a two-stream step like the per-layer updates were"""
    if not items:
        return
    arr = (_lib.BnRunItem * len(items))()
    for a, (coef, rm, rv, mom) in zip(arr, items):
        a.coef, a.running_mean, a.running_var, a.C, a.momentum = coef.data_ptr(), rm.data_ptr(), rv.data_ptr(), coef.shape[1], mom
    with ordered("bn_running_batch"):
        _lib.call("cy_bn_running_update", arr, len(items), _stream())


def bn_finalize_block(partials: Optional[Tensor], count: int, gamma: Optional[Tensor], beta: Optional[Tensor],
                      running_mean: Optional[Tensor], running_var: Optional[Tensor], momentum: float,
                      eps: float, use_batch_stats: bool, update_running: bool, Cc: int, device) -> Tensor:
    """the coefficients of one BatchNorm evaluation from partial rows (or the running statistics): one contiguous
    [4, C] block with rows scale, shift, mean, invstd -- the first four rows of BnState.coef"""
    out = _f32(4 * Cc, device).view(4, Cc)
    npart = 0 if partials is None else partials.shape[0]
    def launch():
        _lib.call("cy_bn_finalize", _ptr(partials), npart, Cc, float(count), _ptr(gamma), _ptr(beta),
                  _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
                  int(use_batch_stats), int(update_running), out[0].data_ptr(), out[1].data_ptr(),
                  out[2].data_ptr(), out[3].data_ptr(), _stream())

    if running_mean is not None and (update_running or not use_batch_stats):
        # reads or updates the running statistics (the batched updates of the accumulator path share the second key)
        with ordered(("bn_running", running_mean.data_ptr())), ordered("bn_running_batch"):
            launch()
    else:
        launch()
    return out


def bn_finalize(*args, **kwargs):
    """`bn_finalize_block` as its four rows: (scale, shift, mean, invstd)"""
    out = bn_finalize_block(*args, **kwargs)
    return out[0], out[1], out[2], out[3]


def bn_relu_apply(y: Tensor, scale: Tensor, shift: Tensor, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    N, Cc, H, W = y.shape
    out_dtype = out_dtype or y.dtype
    out = empty_nhwc(N, Cc, H, W, out_dtype, y.device)
    _lib.call("cy_bn_relu_apply", y.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
              N * H * W, Cc, dtype_code(y.dtype), dtype_code(out_dtype), _stream())
    return out


def bn_relu_apply_pool(y: Tensor, scale: Tensor, shift: Tensor) -> Tuple[Tensor, Tensor]:
    """(relu(scale*y + shift), its 2x2 max) in one pass -- the block output and what nn.MaxPool2d(2) makes of it"""
    N, Cc, H2, W2 = y.shape
    if H2 % 2 or W2 % 2:
        raise ValueError(f"max-pool 2x2 needs even spatial dims, got {H2}x{W2}")
    out = empty_nhwc(N, Cc, H2, W2, y.dtype, y.device)
    pooled = empty_nhwc(N, Cc, H2 // 2, W2 // 2, y.dtype, y.device)
    dt = dtype_code(y.dtype)
    _lib.call("cy_bn_relu_apply_pool", y.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
              pooled.data_ptr(), N, H2 // 2, W2 // 2, Cc, dt, dt, _stream())
    return out, pooled


def _bn_param_grads(Cc: int, dev, dgamma_out: Optional[Tensor], dbeta_out: Optional[Tensor], want: bool):
    """(pg, pb, accumulate, guard): where a BatchNorm backward launch writes dgamma / dbeta -- ADDED into dgamma_out /
    dbeta_out, else into a fresh [2, C] pair if wanted, else nowhere -- and the context its launch runs in (in-place
    accumulation into the parameters' .grad is ordered across streams)"""
    if dgamma_out is not None:
        return dgamma_out, dbeta_out, True, ordered(("bn_grad", dgamma_out.data_ptr()))
    if want:
        gb = _f32(2 * Cc, dev).view(2, Cc)
        return gb[0], gb[1], False, contextlib.nullcontext()
    return None, None, False, contextlib.nullcontext()


def bn_relu_bwd(da: Tensor, y: Tensor, scale: Tensor, shift: Tensor, mean: Tensor, invstd: Tensor,
                batch_stats: bool, dgamma_out: Optional[Tensor] = None, dbeta_out: Optional[Tensor] = None,
                want_param_grads: bool = True, partials: Optional[Tensor] = None):
    """Backward of a = relu(bn(y)): returns (dy, dgamma, dbeta).  With dgamma_out/dbeta_out the
    parameter gradients are ADDED into those buffers (and returned as None).  `partials`: the reduction pass
    was already done by the kernel that produced `da` (maxpool2_bwd_bn)."""
    N, Cc, H, W = y.shape
    npix = N * H * W
    dev = y.device
    dt = dtype_code(y.dtype)
    if da.dtype != y.dtype:
        da = da.to(y.dtype)
    da = to_nhwc(da)
    if partials is not None:
        part, npart = partials, partials.shape[0]
    else:
        npart = _lib.call("cy_bn_bwd_num_partials", npix, Cc)
        part = _f32(npart * 2 * Cc, dev)
        _lib.call("cy_bn_relu_bwd_reduce", da.data_ptr(), Cc, y.data_ptr(), scale.data_ptr(),
                  shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), npix, Cc, dt,
                  _stream())
    coef = _f32(2 * Cc, dev)
    pg, pb, accum, guard = _bn_param_grads(Cc, dev, dgamma_out, dbeta_out, want_param_grads)
    with guard:
        _lib.call("cy_bn_bwd_finalize", part.data_ptr(), npart, Cc, scale.data_ptr(), mean.data_ptr(),
                  invstd.data_ptr(), float(npix), int(batch_stats), _ptr(pg), _ptr(pb), int(accum), coef.data_ptr(),
                  _stream())
    dy = empty_nhwc(N, Cc, H, W, y.dtype, dev)
    _lib.call("cy_bn_relu_bwd_apply", da.data_ptr(), Cc, y.data_ptr(), scale.data_ptr(), shift.data_ptr(),
              coef.data_ptr(), dy.data_ptr(), npix, Cc, dt, _stream())
    return (dy, None, None) if accum else (dy, pg, pb)


POOL_BN_FUSE = os.environ.get("CY_POOL_BN_FUSE", "1") != "0"  # (A/B switch)


def bn_relu_bwd_acc(da: Tensor, y: Tensor, coef: Tensor, batch_stats: bool, dgamma_out: Optional[Tensor] = None,
                    dbeta_out: Optional[Tensor] = None, want_param_grads: bool = True,
                    acc: Optional[BnAccBuf] = None, acc_filled: bool = False):
    """bn_relu_bwd on an accumulator: the reduce launch adds the sums of dz and dz*xhat into `acc` (skipped when the
    kernel that produced `da` already did, `acc_filled`), the apply launch derives (k1, k0) from it and its first
    workgroup adds the parameter gradients -- two launches instead of three.  coef: the forward pass's [5, C]."""
    N, Cc, H, W = y.shape
    npix = N * H * W
    dev = y.device
    dt = dtype_code(y.dtype)
    if da.dtype != y.dtype:
        da = da.to(y.dtype)
    da = to_nhwc(da)
    if acc is None:
        acc = bn_acc_new(Cc, _lib.call("cy_bn_relu_bwd_workgroups", npix, Cc), dev)
    if not acc_filled:
        _lib.call("cy_bn_relu_bwd_reduce_acc", da.data_ptr(), Cc, y.data_ptr(), coef.data_ptr(), acc.ref, npix, Cc, dt,
                  _stream())
    pg, pb, accum, guard = _bn_param_grads(Cc, dev, dgamma_out, dbeta_out, want_param_grads)
    dy = empty_nhwc(N, Cc, H, W, y.dtype, dev)
    with guard:
        _lib.call("cy_bn_relu_bwd_apply_fold", da.data_ptr(), Cc, y.data_ptr(), coef.data_ptr(), acc.ref, float(npix),
                  int(batch_stats), _ptr(pg), _ptr(pb), int(accum), dy.data_ptr(), npix, Cc, dt, _stream())
    return (dy, None, None) if accum else (dy, pg, pb)


def bn_bwd_reduce_acc(da: Tensor, y: Tensor, coef: Tensor, acc: BnAccBuf) -> None:
    """acc += the sums of dz and dz*xhat over (da, y) (the reduce launch of bn_relu_bwd_acc on its own)"""
    N, Cc, H, W = y.shape
    _lib.call("cy_bn_relu_bwd_reduce_acc", da.data_ptr(), Cc, y.data_ptr(), coef.data_ptr(), acc.ref, N * H * W, Cc,
              dtype_code(y.dtype), _stream())


def bn_bwd_acc_new(N: int, Cc: int, H: int, W: int, pooled: bool, device) -> BnAccBuf:
    """a zeroed accumulator for the backward sums of a BatchNorm over [N, C, H, W], sized for whichever kernel will
    fill it (the reduce launch, the pool backward of the block's output, or the upsample backward of its consumer)"""
    wgs = _lib.call("cy_bn_relu_bwd_workgroups", N * H * W, Cc)
    if pooled and POOL_BN_FUSE and H % 2 == 0 and W % 2 == 0:
        wgs = max(wgs, _lib.load().cy_maxpool2_bwd_bn_num_partials(N, H // 2, W // 2, Cc))
    wgs = max(wgs, _lib.load().cy_upsample2_bwd_bn_workgroups(N, H, W, Cc))
    return bn_acc_new(Cc, wgs, device)


def upsample2_bwd_bn_acc(dup: Tensor, y: Tensor, coef: Tensor, acc: BnAccBuf) -> Optional[Tensor]:
    """upsample2_bwd whose result is the dA of relu(bn(y)): that BatchNorm's backward sums are added into `acc`;
    None where the fused form does not apply"""
    N, Cc, H2, W2 = dup.shape
    if _lib.load().cy_upsample2_bwd_bn_workgroups(N, H2 // 2, W2 // 2, Cc) <= 0 or dup.dtype != y.dtype:
        return None
    dx = empty_nhwc(N, Cc, H2 // 2, W2 // 2, dup.dtype, dup.device)
    _lib.call("cy_upsample2_bwd_bn_acc", dup.data_ptr(), Cc, dx.data_ptr(), y.data_ptr(), coef.data_ptr(), acc.ref, N,
              H2 // 2, W2 // 2, Cc, dtype_code(dup.dtype), _stream())
    return dx


def maxpool2_bwd_bn_acc(x: Tensor, dpool: Tensor, add: Optional[Tensor], y: Tensor, coef: Tensor,
                        acc: Optional[BnAccBuf] = None):
    """maxpool2_bwd whose result is the dA of relu(bn(y)), with that BatchNorm's backward sums added into `acc` (a new
    accumulator if None): (dx, acc), or (dx, None) where the fused form does not apply"""
    N, Cc, H2, W2 = x.shape
    npart = _lib.load().cy_maxpool2_bwd_bn_num_partials(N, H2 // 2, W2 // 2, Cc) if POOL_BN_FUSE else 0
    if npart <= 0:
        return maxpool2_bwd(x, dpool, add), None
    dx = empty_nhwc(N, Cc, H2, W2, x.dtype, x.device)
    if acc is None:
        acc = bn_acc_new(Cc, npart, x.device)
    _lib.call("cy_maxpool2_bwd_bn_acc", x.data_ptr(), dpool.data_ptr(), _ptr(add), Cc, dx.data_ptr(), y.data_ptr(),
              coef.data_ptr(), acc.ref, N, H2 // 2, W2 // 2, Cc, dtype_code(x.dtype), _stream())
    return dx, acc


# The data gradient with the BatchNorm + ReLU backward in its load path (cy_conv3x3_dgrad_bn): one launch instead of
# cy_bn_relu_bwd_apply_fold + cy_conv3x3_fwd; dy comes back as a second output for the weight gradient.  OFF unless
# CY_DGRAD_BN=1: measured per layer (tools/bench_dgrad_bn.py) and in the step (tools/ab.sh CY_DGRAD_BN 0 1) it does not
# pay -- every cout block of a tile, and every tile for its halo, repeats the in-LDS pass over (dA, y) that the apply
# launch does once per element; on the 128-cout tilings the fused launch is 3-5 us shorter than the two it replaces, on
# the 64-cout tilings 5-13 us longer, and the step does not move (6.51 against 6.51 ms with the 128-cout layers fused,
# 6.38 against 6.25 with all of them).  DESIGN.md section 3 "Round 4".
DGRAD_BN = os.environ.get("CY_DGRAD_BN", "0") == "1"


def _dgrad_bn_desc(da: Tensor, Cin: int, split: Optional[int]):
    N, Cc, H, W = da.shape
    dt = dtype_code(da.dtype)
    if split:
        return _desc(N, H, W, Cc, 0, Cin, 0, 2, dt, Cc, 0, split, split, Cin - split)
    return _desc(N, H, W, Cc, 0, Cin, 0, 2, dt, Cc, 0, Cin)


def conv3x3_dgrad_bn_ok(da: Tensor, Cin: int, split: Optional[int] = None) -> bool:
    """does this layer geometry have a launch plan that takes the fused form?"""
    if not (DGRAD_BN and BN_ACC) or da.dtype not in HALF_TYPES or not is_nhwc(da):
        return False
    d = _dgrad_bn_desc(da, Cin, split)
    if d.dgrad_bn is None:
        d.dgrad_bn = bool(_lib.call("cy_conv3x3_dgrad_bn_ok", d.ref))
    return d.dgrad_bn


def conv3x3_dgrad_bn(da: Tensor, y: Tensor, coef: Tensor, acc: "BnAccBuf", batch_stats: bool, wd: Tensor, Cin: int, *,
                     dgamma_out: Optional[Tensor] = None, dbeta_out: Optional[Tensor] = None,
                     want_param_grads: bool = True, split: Optional[int] = None):
    """(dx or (dx1, dx2), dy, dgamma, dbeta): dy = the BatchNorm + ReLU backward of da (formed in the conv's load path
    from da, y and the sums in `acc`), dx = conv3x3(dy, wd).  coef: the forward pass's coefficient block, taken
    by its address."""
    N, Cc, H, W = y.shape
    dev = y.device
    d = _dgrad_bn_desc(da, Cin, split)
    if split:
        out = empty_nhwc(N, split, H, W, y.dtype, dev)
        out2 = empty_nhwc(N, Cin - split, H, W, y.dtype, dev)
    else:
        out, out2 = empty_nhwc(N, Cin, H, W, y.dtype, dev), None
    dy = empty_nhwc(N, Cc, H, W, y.dtype, dev)
    pg, pb, accum, guard = _bn_param_grads(Cc, dev, dgamma_out, dbeta_out, want_param_grads)
    if d.fwd_ws is None:
        d.fwd_ws = _lib.load().cy_conv3x3_fwd_ws_bytes(d.ref)
    nbytes = d.fwd_ws
    ws = _ws(nbytes, dev) if nbytes else None
    bn = _lib.BnBwdIn(y.data_ptr(), coef.data_ptr(), C.pointer(acc.s), float(N * H * W), int(batch_stats), int(accum),
                      _ptr(pg), _ptr(pb), dy.data_ptr())
    ev = _prof_begin()
    with guard:
        _lib.call("cy_conv3x3_dgrad_bn", d.ref, da.data_ptr(), C.byref(bn), wd.data_ptr(), out.data_ptr(), _ptr(out2),
                  _ptr(ws), nbytes, _stream())
    if ev is not None:
        esz = y.element_size()
        nb = esz * (3 * y.numel() + N * H * W * Cin + 9 * Cc * Cin)
        _prof_end(ev, "conv3x3_fwd_dgrad", 2.0 * N * H * W * 9 * Cc * Cin, float(nb))
    dx = (out, out2) if split else out
    return (dx, dy, None, None) if accum else (dx, dy, pg, pb)


# A data gradient whose output is the dA of a BatchNorm + ReLU adds that layer's backward sums in its epilogue
# (cy_conv3x3_dgrad_dz): the reduce launch over (dA, y) goes.  OFF unless CY_DGRAD_DZ=1: on the 16-row tilings the fused
# launch takes what the two took (28.0 against 20.6 + 7.5 us at 56 x 56 x 128, tools/bench_dgrad_dz.py), on the tilings
# with four fragments per wave the sums' working set spills ~900 registers (3-4 x slower: excluded by the plan), and the
# step does not move (tools/ab.sh CY_DGRAD_DZ 0 1: 6.28 against 6.28 ms) -- the conv kernels are what the step waits for,
# work moved into them costs what it saved.  DESIGN.md section 3 "Round 4".
DGRAD_DZ = os.environ.get("CY_DGRAD_DZ", "0") == "1"
_dz_ok_cache = {}


def conv3x3_dgrad_dz_ok(dy: Tensor, Cin: int, split: Optional[int], c0: int, Cs: int) -> bool:
    if not (DGRAD_DZ and BN_ACC) or dy.dtype not in HALF_TYPES:
        return False
    N, Cc, H, W = dy.shape
    key = (N, Cc, H, W, Cin, split, c0, Cs, dy.dtype)
    ok = _dz_ok_cache.get(key)
    if ok is None:
        dt = dtype_code(dy.dtype)
        d = _desc(N, H, W, Cc, 0, Cin, 0, 0, dt, Cc, 0, split, split, Cin - split) if split else \
            _desc(N, H, W, Cc, 0, Cin, 0, 0, dt, Cc, 0, Cin)
        ok = _dz_ok_cache[key] = bool(_lib.call("cy_conv3x3_dgrad_dz_ok", d.ref, c0, Cs))
    return ok


def conv3x3_dgrad_dz(dy: Tensor, wd: Tensor, Cin: int, y: Tensor, coef: Tensor, acc: "BnAccBuf", *,
                     split: Optional[int] = None):
    """conv3x3_fwd(dy, wd) as a data gradient whose output -- all of it, or with `split` its second part -- is the dA
    of relu(bn(y)): that layer's backward sums are added into `acc` by the epilogue.  Returns out or (out1, out2)."""
    N, Cc, H, W = dy.shape
    dev = dy.device
    dt = dtype_code(dy.dtype)
    if split:
        out = empty_nhwc(N, split, H, W, dy.dtype, dev)
        out2 = empty_nhwc(N, Cin - split, H, W, dy.dtype, dev)
        d = _desc(N, H, W, Cc, 0, Cin, 0, 0, dt, Cc, 0, split, split, Cin - split)
    else:
        out, out2 = empty_nhwc(N, Cin, H, W, dy.dtype, dev), None
        d = _desc(N, H, W, Cc, 0, Cin, 0, 0, dt, Cc, 0, Cin)
    if d.fwd_ws is None:
        d.fwd_ws = _lib.load().cy_conv3x3_fwd_ws_bytes(d.ref)
    nbytes = d.fwd_ws
    ws = _ws(nbytes, dev) if nbytes else None
    dz = _lib.BnDzOut(y.data_ptr(), coef.data_ptr(), C.pointer(acc.s), split or 0, y.shape[1])
    ev = _prof_begin()
    _lib.call("cy_conv3x3_dgrad_dz", d.ref, dy.data_ptr(), wd.data_ptr(), out.data_ptr(), _ptr(out2), C.byref(dz),
              _ptr(ws), nbytes, _stream())
    if ev is not None:
        esz = dy.element_size()
        nb = esz * (dy.numel() + y.numel() + N * H * W * Cin + 9 * Cc * Cin)
        _prof_end(ev, "conv3x3_fwd_dgrad", 2.0 * N * H * W * 9 * Cc * Cin, float(nb))
    return (out, out2) if split else out


def maxpool2_bwd(x: Tensor, dpool: Tensor, add: Optional[Tensor] = None) -> Tensor:
    N, Cc, H2, W2 = x.shape
    dx = empty_nhwc(N, Cc, H2, W2, x.dtype, x.device)
    _lib.call("cy_maxpool2_bwd", x.data_ptr(), dpool.data_ptr(), _ptr(add), Cc, dx.data_ptr(), N,
              H2 // 2, W2 // 2, Cc, dtype_code(x.dtype), _stream())
    return dx


def maxpool2_bwd_bn(x: Tensor, dpool: Tensor, add: Optional[Tensor], y: Tensor, scale: Tensor, shift: Tensor,
                    mean: Tensor, invstd: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """maxpool2_bwd whose result is the dA of relu(bn(y)): (dx, partial rows [P, 2, C] of that BatchNorm's backward
    sums), or (dx, None) where the fused form does not apply (channel groups that do not divide a workgroup)"""
    N, Cc, H2, W2 = x.shape
    npart = _lib.load().cy_maxpool2_bwd_bn_num_partials(N, H2 // 2, W2 // 2, Cc) if POOL_BN_FUSE else 0
    if npart <= 0:
        return maxpool2_bwd(x, dpool, add), None
    dx = empty_nhwc(N, Cc, H2, W2, x.dtype, x.device)
    part = _f32(npart * 2 * Cc, x.device).view(npart, 2, Cc)
    _lib.call("cy_maxpool2_bwd_bn", x.data_ptr(), dpool.data_ptr(), _ptr(add), Cc, dx.data_ptr(), y.data_ptr(),
              scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), N,
              H2 // 2, W2 // 2, Cc, dtype_code(x.dtype), _stream())
    return dx, part


def upsample2_bwd(dup: Tensor) -> Tensor:
    N, Cc, H2, W2 = dup.shape
    dx = empty_nhwc(N, Cc, H2 // 2, W2 // 2, dup.dtype, dup.device)
    _lib.call("cy_upsample2_bwd", dup.data_ptr(), Cc, dx.data_ptr(), N, H2 // 2, W2 // 2, Cc,
              dtype_code(dup.dtype), _stream())
    return dx


def norm_act_plan(kind: str, N: int, H: int, W: int, Cc: int, dtype: torch.dtype = torch.float32, fold: int = 0,
                  out_dtype: Optional[torch.dtype] = None) -> dict:
    """the launch plan of the BatchNorm, pool and upsample kernels (cy_norm_act_plan; host-side query, no GPU needed).
    kind: one of _lib.NORM_ACT_KINDS; (H, W) are the pooled / low-resolution dims for the pool and upsample kinds, and
    N * H * W the number of partial rows for the finalize kinds.  fold: 0, or the replica count R of the accumulator the
    launch reads or adds into.  Returns the fields of cy_norm_act_plan_t; "status" is what the launch answers for the
    shape (0, or CY_ERR_SHAPE / CY_ERR_DTYPE), so refused shapes do not raise here."""
    dt = dtype_code(dtype)
    if out_dtype is not None and out_dtype != dtype:
        dt |= (dtype_code(out_dtype) + 1) << 4
    return _query(_lib.NormActPlan, "cy_norm_act_plan", _lib.NORM_ACT_KINDS.index(kind), int(N), int(H), int(W), int(Cc),
                  dt, int(fold))


# --------------------------------------------------------------------------- head + losses
def head_fwd(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Tensor:
    """x [N,C,H,W] NHWC -> f32 logits [N,K,H,W] NHWC."""
    require_gpu(x, w)
    N, Cc, H, W = x.shape
    K = w.shape[0]
    logits = empty_nhwc(N, K, H, W, torch.float32, x.device)
    w2 = w.detach().reshape(K, Cc).float().contiguous()
    _lib.call("cy_head1x1_fwd", x.data_ptr(), w2.data_ptr(), _ptr(None if b is None else b.detach()),
              logits.data_ptr(), N * H * W, Cc, K, dtype_code(x.dtype), _stream())
    return logits


def head_plan(npix: int, C_in: int, K: int, need_dx: bool = True, need_dw: bool = True) -> dict:
    """the launch plan of cy_head1x1_fwd / _bwd for npix pixels, C_in channels, K outputs (host-side query, no GPU
    needed): the fields of cy_head_plan, and "ws_bytes", the backward's workspace (0 without need_dw).  Shapes the
    kernels refuse raise HipKernelError (CY_ERR_SHAPE)."""
    out = _query(_lib.HeadPlan, "cy_head1x1_plan", int(npix), int(C_in), int(K), int(bool(need_dx)), int(bool(need_dw)))
    out["ws_bytes"] = int(_lib.load().cy_head1x1_bwd_ws_bytes(int(npix), int(C_in), int(K))) if need_dw else 0
    return out


def head_bwd(x: Tensor, w: Tensor, dlogits: Tensor, need_dx: bool, need_dw: bool,
             dw_into: Optional[Tensor] = None, db_into: Optional[Tensor] = None):
    """(dx, dw, db); with dw_into (and db_into for a head with bias) the parameter gradients are ADDED into those live
    .grad buffers by the reduction kernel and returned as None"""
    N, Cc, H, W = x.shape
    K = w.shape[0]
    npix = N * H * W
    dlogits = to_nhwc(dlogits.float())
    w2 = w.detach().reshape(K, Cc).float().contiguous()
    dx = empty_nhwc(N, Cc, H, W, x.dtype, x.device) if need_dx else None
    dw = db = None
    nbytes = 0
    ws = None
    if need_dw:
        nbytes = _lib.load().cy_head1x1_bwd_ws_bytes(npix, Cc, K)
        ws = _ws(nbytes, x.device)
        if dw_into is not None:
            with ordered(("head_grad", dw_into.data_ptr())):
                _lib.call("cy_head1x1_bwd_into", x.data_ptr(), w2.data_ptr(), dlogits.data_ptr(), _ptr(dx),
                          dw_into.data_ptr(), _ptr(db_into), npix, Cc, K, dtype_code(x.dtype), _ptr(ws), nbytes, _stream())
            return dx, None, None
        dw = _f32(K * Cc, x.device)
        db = _f32(K, x.device)
    _lib.call("cy_head1x1_bwd", x.data_ptr(), w2.data_ptr(), dlogits.data_ptr(), _ptr(dx), _ptr(dw),
              _ptr(db), npix, Cc, K, dtype_code(x.dtype), _ptr(ws), nbytes, _stream())
    if dw is not None:
        dw = dw.view(K, Cc, 1, 1)
    return dx, dw, db


def softmax_kl_fwd(logits: Tensor, target: Tensor, eps: float) -> Tensor:
    N, K, H, W = logits.shape
    npix = N * H * W
    nbytes = _lib.load().cy_softmax_kl_ws_bytes(npix)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_softmax_kl_fwd", logits.data_ptr(), target.data_ptr(), loss.data_ptr(), npix, K,
              float(eps), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_kl_bwd(logits: Tensor, target: Tensor, gscale: Tensor, eps: float) -> Tensor:
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_kl_bwd", logits.data_ptr(), target.data_ptr(), gscale.data_ptr(),
              d.data_ptr(), N * H * W, K, float(eps), _stream())
    return d


def _class_weight(logits: Tensor, weight: Optional[Tensor]) -> Optional[Tensor]:
    """the [K] f32 class weights the cy_softmax_wkl_* entries read, on the logits' device; None: all ones"""
    if weight is None:
        return None
    assert weight.dim() == 1 and weight.shape[0] == logits.shape[1], (tuple(weight.shape), tuple(logits.shape))
    assert weight.device == logits.device, (weight.device, logits.device)
    return weight.detach().float().contiguous()


def softmax_wkl_fwd(logits: Tensor, target: Tensor, weight: Optional[Tensor], eps: float, reduction: str) -> Tensor:
    """sum_pix -w[y] log((softmax(z)_y + eps) / (1 + eps)) over npix ("mean") or 1 ("sum"): a device scalar; "none":
    the [N, H, W] map (one launch)"""
    N, K, H, W = logits.shape
    npix = N * H * W
    weight = _class_weight(logits, weight)
    if reduction == "none":
        out = _f32(npix, logits.device)
        _lib.call("cy_softmax_wkl_map_fwd", logits.data_ptr(), target.data_ptr(), _ptr(weight), out.data_ptr(), npix, K,
                  float(eps), _stream())
        return out.view(N, H, W)
    nbytes = _lib.load().cy_softmax_wkl_ws_bytes(npix)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_softmax_wkl_fwd", logits.data_ptr(), target.data_ptr(), _ptr(weight), loss.data_ptr(), npix, K,
              float(eps), float(npix if reduction == "mean" else 1), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_wkl_bwd(logits: Tensor, target: Tensor, weight: Optional[Tensor], up: Tensor, eps: float,
                    reduction: str) -> Tensor:
    """`up`: the upstream gradient on the device, f32 [1] ("mean", "sum") or the contiguous [N, H, W] map ("none")"""
    N, K, H, W = logits.shape
    npix = N * H * W
    weight = _class_weight(logits, weight)
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    if reduction == "none":
        assert up.numel() == npix and up.is_contiguous() and up.dtype == torch.float32, (tuple(up.shape), up.dtype)
        _lib.call("cy_softmax_wkl_map_bwd", logits.data_ptr(), target.data_ptr(), _ptr(weight), up.data_ptr(),
                  d.data_ptr(), npix, K, float(eps), _stream())
    else:
        _lib.call("cy_softmax_wkl_bwd", logits.data_ptr(), target.data_ptr(), _ptr(weight), up.data_ptr(),
                  d.data_ptr(), npix, K, float(eps), float(npix if reduction == "mean" else 1), _stream())
    return d


DICE_REDUCTIONS = ("mean", "sum", "none")  # the `reduction` codes of cy_softmax_dice_*


def softmax_dice_fwd(logits: Tensor, target: Tensor, p: int, smooth: float, ignore: Optional[int], reduction: str):
    """-> (result: a device scalar, or [N] for "none"; table: f64 [N, K, 2] = {num, den}, which the backward reads)"""
    N, K, H, W = logits.shape
    nbytes = _lib.load().cy_softmax_dice_ws_bytes(N, H * W, K)
    ws = _ws(nbytes, logits.device)
    table = torch.empty((N, K, 2), dtype=torch.float64, device=logits.device)
    res = _f32(N if reduction == "none" else 1, logits.device)
    _lib.call("cy_softmax_dice_fwd", logits.data_ptr(), target.data_ptr(), table.data_ptr(), res.data_ptr(), N, H * W,
              K, int(p), float(smooth), -1 if ignore is None else int(ignore), DICE_REDUCTIONS.index(reduction),
              ws.data_ptr(), nbytes, _stream())
    return (res if reduction == "none" else res.view(())), table


def softmax_dice_bwd(logits: Tensor, target: Tensor, table: Tensor, up: Tensor, p: int, ignore: Optional[int],
                     reduction: str) -> Tensor:
    """`up`: the upstream gradient on the device, f32 [1] ("mean", "sum") or [N] ("none")"""
    N, K, H, W = logits.shape
    assert up.numel() == (N if reduction == "none" else 1) and up.is_contiguous() and up.dtype == torch.float32
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_dice_bwd", logits.data_ptr(), target.data_ptr(), table.data_ptr(), up.data_ptr(),
              d.data_ptr(), N, H * W, K, int(p), -1 if ignore is None else int(ignore),
              DICE_REDUCTIONS.index(reduction), _stream())
    return d


def softmax_mse_fwd(a: Tensor, b: Tensor) -> Tensor:
    N, K, H, W = a.shape
    npix = N * H * W
    nbytes = _lib.load().cy_softmax_mse_ws_bytes(npix)
    ws = _ws(nbytes, a.device)
    loss = _f32(1, a.device)
    _lib.call("cy_softmax_mse_fwd", a.data_ptr(), b.data_ptr(), loss.data_ptr(), npix, K,
              ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_mse_bwd(a: Tensor, b: Tensor, gscale: Tensor, need_a: bool, need_b: bool):
    N, K, H, W = a.shape
    da = empty_nhwc(N, K, H, W, torch.float32, a.device) if need_a else None
    db = empty_nhwc(N, K, H, W, torch.float32, a.device) if need_b else None
    _lib.call("cy_softmax_mse_bwd", a.data_ptr(), b.data_ptr(), gscale.data_ptr(), _ptr(da), _ptr(db),
              N * H * W, K, _stream())
    return da, db


def softmax_group_kl_fwd(logits: Tensor, target: Tensor, G: int, eps: float) -> Tensor:
    """mean_p -log((P_p + eps) / (1 + eps)), P_p = the softmax mass of the target class's K/G contiguous channels"""
    N, K, H, W = logits.shape
    npix = N * H * W
    nbytes = _lib.load().cy_softmax_group_kl_ws_bytes(npix, K)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_softmax_group_kl_fwd", logits.data_ptr(), target.data_ptr(), loss.data_ptr(), npix, K, int(G),
              float(eps), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_group_kl_bwd(logits: Tensor, target: Tensor, gscale: Tensor, G: int, eps: float) -> Tensor:
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_group_kl_bwd", logits.data_ptr(), target.data_ptr(), gscale.data_ptr(), d.data_ptr(),
              N * H * W, K, int(G), float(eps), _stream())
    return d


def _mix_arg(logits: Tensor, mix: Tensor) -> Tensor:
    """the [K, C] f32 mixing matrix the cy_softmax_mix_* entries read, on the logits' device"""
    assert mix.dim() == 2 and mix.shape[0] == logits.shape[1], (tuple(mix.shape), tuple(logits.shape))
    assert mix.device == logits.device, (mix.device, logits.device)
    return mix.detach().float().contiguous()


def softmax_mix_kl_fwd(logits: Tensor, target: Tensor, mix: Tensor, eps: float) -> Tensor:
    """mean_p -log((R_p + eps) / (1 + eps)), R_p = sum_k softmax(z_p)_k mix[k, t_p]; mix is [K, C]"""
    N, K, H, W = logits.shape
    mix = _mix_arg(logits, mix)
    npix = N * H * W
    nbytes = _lib.load().cy_softmax_mix_kl_ws_bytes(npix, K)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_softmax_mix_kl_fwd", logits.data_ptr(), target.data_ptr(), mix.data_ptr(), loss.data_ptr(), npix, K,
              mix.shape[1], float(eps), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_mix_kl_bwd(logits: Tensor, target: Tensor, mix: Tensor, gscale: Tensor, eps: float, need_mix: bool):
    """-> (dlogits, dmix or None); dmix [K, C] only where `need_mix` (it costs the per-block partials and a launch)"""
    N, K, H, W = logits.shape
    mix = _mix_arg(logits, mix)
    C = mix.shape[1]
    npix = N * H * W
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    dmix, ws, nbytes = None, None, 0
    if need_mix:
        dmix = _f32(K * C, logits.device).view(K, C)
        nbytes = _lib.load().cy_softmax_mix_kl_bwd_ws_bytes(npix, K, C)
        ws = _ws(nbytes, logits.device)
    _lib.call("cy_softmax_mix_kl_bwd", logits.data_ptr(), target.data_ptr(), mix.data_ptr(), gscale.data_ptr(),
              d.data_ptr(), _ptr(dmix), npix, K, C, float(eps), _ptr(ws), nbytes, _stream())
    return d, dmix


# The four regularisers below (entropy, self-MSE, UA-MT, ICT's mix-MSE) have two sets of entry points with the same
# arguments: one thread per pixel up to 16 classes (csrc/cy_pixel_reg.hip, csrc/cy_mixup.hip) and sixteen lanes per
# pixel for multi-prototype logits, 16 < K <= 64 (csrc/cy_wide_reg.hip).  Any other K goes to the first set, whose
# refusal is the error the caller sees.
WIDE_REG_KMIN, WIDE_REG_KMAX = 17, 64
WIDE_REG_FAMILIES = {"entropy": _lib.CY_WIDE_ENTROPY, "selfmse": _lib.CY_WIDE_SELFMSE, "uamt": _lib.CY_WIDE_UAMT,
                     "mixmse": _lib.CY_WIDE_MIXMSE}


def wide_reg_plan(family: str, npix: int, K: int, align: int = 16) -> dict:
    """the launch rule of the wide-K regularisers (host-side query, no GPU needed): the values of cy_wide_reg_plan by
    name.  `align`: the bytes every base pointer of the call is aligned to.  What the launches refuse raises
    HipKernelError with their status."""
    return _query(_lib.WideRegPlan, "cy_wide_reg_plan", WIDE_REG_FAMILIES[family], int(npix), int(K), int(align))


def _by_k(name: str, K: int) -> str:
    """'softmax_entropy' -> the stem of its entry points for K classes"""
    return f"cy_{name}_row" if WIDE_REG_KMIN <= K <= WIDE_REG_KMAX else f"cy_{name}"


def _pixel_loss_fwd(name: str, x: Tensor, out: int = 1):
    """what the forward of a pixel-wise regulariser (csrc/cy_pixel_reg.hip, csrc/cy_wide_reg.hip) takes: (its entry
    point, npix, K, workspace, its bytes, the `out` device floats of the result)"""
    N, K, H, W = x.shape
    npix = N * H * W
    stem = _by_k(name, K)
    nbytes = getattr(_lib.load(), f"{stem}_ws_bytes")(npix)
    ws = _ws(nbytes, x.device)
    res = _f32(out, x.device)
    return f"{stem}_fwd", npix, K, ws, nbytes, res


def softmax_entropy_fwd(logits: Tensor, eps: float) -> Tensor:
    entry, npix, K, ws, nbytes, loss = _pixel_loss_fwd("softmax_entropy", logits)
    _lib.call(entry, logits.data_ptr(), loss.data_ptr(), npix, K, float(eps), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_entropy_bwd(logits: Tensor, gscale: Tensor, eps: float) -> Tensor:
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call(_by_k("softmax_entropy", K) + "_bwd", logits.data_ptr(), gscale.data_ptr(), d.data_ptr(), N * H * W, K,
              float(eps), _stream())
    return d


def softmax_selfmse_fwd(logits: Tensor) -> Tensor:
    entry, npix, K, ws, nbytes, loss = _pixel_loss_fwd("softmax_selfmse", logits)
    _lib.call(entry, logits.data_ptr(), loss.data_ptr(), npix, K, ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_selfmse_bwd(logits: Tensor, gscale: Tensor) -> Tensor:
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call(_by_k("softmax_selfmse", K) + "_bwd", logits.data_ptr(), gscale.data_ptr(), d.data_ptr(), N * H * W, K,
              _stream())
    return d


def uamt_mse_fwd(teacher: Tensor, student: Tensor, thr: float, hard: bool) -> Tensor:
    """-> device f32 [2] = (loss, mask_mean)"""
    entry, npix, K, ws, nbytes, res = _pixel_loss_fwd("uamt_mse", teacher, out=2)
    _lib.call(entry, teacher.data_ptr(), student.data_ptr(), res.data_ptr(), npix, K, float(thr), int(bool(hard)),
              ws.data_ptr(), nbytes, _stream())
    return res


def uamt_mse_bwd(teacher: Tensor, student: Tensor, result: Tensor, gscale: Tensor, thr: float, hard: bool) -> Tensor:
    N, K, H, W = student.shape
    d = empty_nhwc(N, K, H, W, torch.float32, student.device)
    _lib.call(_by_k("uamt_mse", K) + "_bwd", teacher.data_ptr(), student.data_ptr(), result.data_ptr(),
              gscale.data_ptr(), d.data_ptr(), N * H * W, K, float(thr), int(bool(hard)), _stream())
    return d


# --------------------------------------------------------------------------- IMSAT (csrc/cy_imsat.hip)
IMSAT_EPS = 1e-8  # the module-level entropy_criterion of semi_seg/hooks/midl.py:13
IMSAT_FORMS = {"rows": _lib.CY_IMSAT_ROWS, "pair": _lib.CY_IMSAT_PAIR, "logits": _lib.CY_IMSAT_LOGITS}
IMSAT_LOGITS_KMAX = 16  # classes of cy_softmax_imsat_*


def imsat_plan(form: str, R: int, K: int, align: int = 16) -> dict:
    """the launch rule of the IMSAT kernels (host-side query, no GPU needed): the values of cy_imsat_plan by name, and
    "ws_bytes", the forward's workspace.  `align`: the bytes every base pointer of the call is aligned to.  What the
    launches refuse raises HipKernelError with their status."""
    out = _query(_lib.ImsatPlan, "cy_imsat_plan", IMSAT_FORMS[form], int(R), int(K), int(align))
    query = {"rows": "cy_imsat_ws_bytes", "pair": "cy_imsat_pair_ws_bytes", "logits": "cy_softmax_imsat_ws_bytes"}
    out["ws_bytes"] = int(getattr(_lib.load(), query[form])(int(R), int(K)))
    return out


def _imsat_outputs(nin: int, K: int, device, out: Optional[Tensor], coef: Optional[Tensor], mean: Optional[Tensor]):
    out = _f32(5 if nin == 2 else 2, device) if out is None else out
    coef = _f32(nin * K, device) if coef is None else coef
    mean = _f32(nin * K, device) if mean is None else mean
    return out, coef, mean


def imsat_fwd(p: Tensor, out: Optional[Tensor] = None, coef: Optional[Tensor] = None, mean: Optional[Tensor] = None):
    """p: f32 [R, K] contiguous probability rows (any 4-byte aligned base) -> (out [2] = {marg, cond}, coef [K], mean
    [K]); the three results may be given as contiguous f32 views to write into"""
    require_gpu(p)
    R, K = p.shape
    out, coef, mean = _imsat_outputs(1, K, p.device, out, coef, mean)
    nbytes = _lib.load().cy_imsat_ws_bytes(R, K)
    ws = _ws(nbytes, p.device)
    _lib.call("cy_imsat_fwd", p.data_ptr(), out.data_ptr(), coef.data_ptr(), mean.data_ptr(), R, K, IMSAT_EPS,
              ws.data_ptr(), nbytes, _stream())
    return out, coef, mean


def imsat_bwd(p: Tensor, coef: Tensor, g: Tensor, dp: Optional[Tensor] = None) -> Tensor:
    """g: device f32 [2], the upstream gradients of (marg, cond) -> dp [R, K]"""
    R, K = p.shape
    dp = _f32(R * K, p.device).view(R, K) if dp is None else dp
    _lib.call("cy_imsat_bwd", p.data_ptr(), coef.data_ptr(), g.data_ptr(), dp.data_ptr(), R, K, IMSAT_EPS, _stream())
    return dp


def imsat_pair_fwd(x1: Tensor, x2: Tensor, out: Optional[Tensor] = None, coef: Optional[Tensor] = None,
                   mean: Optional[Tensor] = None):
    """x1, x2: f32 [R, K] contiguous -> (out [5] = {marg1, cond1, marg2, cond2, mse}, coef [2, K], mean [2, K])"""
    require_gpu(x1, x2)
    R, K = x1.shape
    assert x2.shape == x1.shape, (x1.shape, x2.shape)
    out, coef, mean = _imsat_outputs(2, K, x1.device, out, coef, mean)
    nbytes = _lib.load().cy_imsat_pair_ws_bytes(R, K)
    ws = _ws(nbytes, x1.device)
    _lib.call("cy_imsat_pair_fwd", x1.data_ptr(), x2.data_ptr(), out.data_ptr(), coef.data_ptr(), mean.data_ptr(), R, K,
              IMSAT_EPS, ws.data_ptr(), nbytes, _stream())
    return out, coef.view(2, K), mean.view(2, K)


def imsat_pair_bwd(x1: Tensor, x2: Tensor, coef: Tensor, g: Tensor, d1: Optional[Tensor] = None,
                   d2: Optional[Tensor] = None):
    """g: device f32 [5], the upstream gradients in the order of `out` -> (dx1, dx2)"""
    R, K = x1.shape
    d1 = _f32(R * K, x1.device).view(R, K) if d1 is None else d1
    d2 = _f32(R * K, x1.device).view(R, K) if d2 is None else d2
    _lib.call("cy_imsat_pair_bwd", x1.data_ptr(), x2.data_ptr(), coef.data_ptr(), g.data_ptr(), d1.data_ptr(),
              d2.data_ptr(), R, K, IMSAT_EPS, _stream())
    return d1, d2


def softmax_imsat_fwd(logits: Tensor, out: Optional[Tensor] = None, coef: Optional[Tensor] = None,
                      mean: Optional[Tensor] = None):
    """logits: f32 [N, K, H, W] with NHWC memory, K <= 16 -> as imsat_fwd, of softmax(logits, 1)"""
    require_gpu(logits)
    N, K, H, W = logits.shape
    out, coef, mean = _imsat_outputs(1, K, logits.device, out, coef, mean)
    nbytes = _lib.load().cy_softmax_imsat_ws_bytes(N * H * W, K)
    ws = _ws(nbytes, logits.device)
    _lib.call("cy_softmax_imsat_fwd", logits.data_ptr(), out.data_ptr(), coef.data_ptr(), mean.data_ptr(), N * H * W, K,
              IMSAT_EPS, ws.data_ptr(), nbytes, _stream())
    return out, coef, mean


def softmax_imsat_bwd(logits: Tensor, coef: Tensor, g: Tensor) -> Tensor:
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_imsat_bwd", logits.data_ptr(), coef.data_ptr(), g.data_ptr(), d.data_ptr(), N * H * W, K,
              IMSAT_EPS, _stream())
    return d


# --------------------------------------------------------------------------- MixUp and ICT (csrc/cy_mixup.hip)
MIX_FORMS = {"images": _lib.CY_MIX_IMAGES, "mixkl": _lib.CY_MIX_KL, "mixmse": _lib.CY_MIX_MSE}


def mix_plan(form: str, N: int, per_image: int, K: int = 0, align: int = 16) -> dict:
    """the launch rule of the mixing kernels (host-side query, no GPU needed): the values of cy_mix_plan by name.
    `per_image`: the elements of an image (form "images") or its pixels (the losses).  What the launches refuse raises
    HipKernelError with their status."""
    return _query(_lib.MixPlan, "cy_mix_plan", MIX_FORMS[form], int(N), int(per_image), int(K), int(align))


def mix_weights(lam: float) -> Tuple[float, float]:
    """(w_self, w_other) = lam and 1 - lam, formed in f64 as `lam * x + (1 - lam) * x[index]` forms them; ctypes
    rounds each to f32 at the call, as torch does when it multiplies an f32 tensor by a Python scalar"""
    lam = float(lam)
    return lam, 1.0 - lam


def mix_index(index: Tensor, N: int, device) -> Tensor:
    """the int32 [N] device copy of a mixing index the kernels read.  `index` is a CPU integer tensor (what
    torch.randperm gives); any values in [0, N) are allowed, one outside raises ValueError before anything is uploaded
    or launched.  A CUDA int32 tensor is taken as the result of an earlier call and returned as it is."""
    if index.is_cuda and index.dtype == torch.int32 and index.shape == (N,):
        return index
    if index.is_cuda or index.is_floating_point() or index.dtype == torch.bool:
        raise TypeError(f"mixing index: expected a CPU integer tensor, got {index.dtype} on {index.device}")
    if index.shape != (N,):
        raise ValueError(f"mixing index: expected shape ({N},), got {tuple(index.shape)}")
    if N and (int(index.min()) < 0 or int(index.max()) >= N):
        raise ValueError(f"mixing index: values must lie in [0, {N}), got {index.tolist()}")
    return pinned.upload(index.to(torch.int32), device)


def mix_images(x: Tensor, index: Tensor, w_self: float, w_other: float) -> Tensor:
    """w_self * x + w_other * x[index] over the leading dimension of an f32 tensor, in x's memory format: bit-equal to
    torch's CPU f32 evaluation of that expression.  No gradient is recorded (images and targets carry none)."""
    require_gpu(x)
    assert x.dtype == torch.float32 and x.dim() >= 1, (x.dtype, tuple(x.shape))
    N = x.shape[0]
    idx = mix_index(index, N, x.device)
    x = x.detach()
    if not (x.is_contiguous() or (x.dim() == 4 and is_nhwc(x))):
        x = x.contiguous()
    out = torch.empty_like(x)
    if x.numel():
        _lib.call("cy_mix_images", x.data_ptr(), idx.data_ptr(), float(w_self), float(w_other), out.data_ptr(), N,
                  x.numel() // N, _stream())
    return out


def softmax_mixkl_fwd(logits: Tensor, target: Tensor, index: Tensor, w_self: float, w_other: float,
                      eps: float) -> Tensor:
    """logits f32 [N,K,H,W] with NHWC memory, target int64 [N,H,W] contiguous -> device scalar: KL_div(eps) of
    softmax(logits) against w_self * onehot(target) + w_other * onehot(target)[index]"""
    N, K, H, W = logits.shape
    idx = mix_index(index, N, logits.device)
    nbytes = _lib.load().cy_softmax_mixkl_ws_bytes(N, H * W)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_softmax_mixkl_fwd", logits.data_ptr(), target.data_ptr(), idx.data_ptr(), float(w_self),
              float(w_other), loss.data_ptr(), N, H * W, K, float(eps), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_mixkl_bwd(logits: Tensor, target: Tensor, index: Tensor, w_self: float, w_other: float, gscale: Tensor,
                      eps: float) -> Tensor:
    N, K, H, W = logits.shape
    idx = mix_index(index, N, logits.device)
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_mixkl_bwd", logits.data_ptr(), target.data_ptr(), idx.data_ptr(), float(w_self),
              float(w_other), gscale.data_ptr(), d.data_ptr(), N, H * W, K, float(eps), _stream())
    return d


def softmax_mixmse_fwd(student: Tensor, teacher: Tensor, index: Tensor, w_self: float, w_other: float) -> Tensor:
    """student, teacher: f32 logits [N,K,H,W] with NHWC memory -> device scalar: the mean of (softmax(student) -
    (w_self * softmax(teacher) + w_other * softmax(teacher)[index]))^2"""
    N, K, H, W = student.shape
    assert teacher.shape == student.shape, (tuple(teacher.shape), tuple(student.shape))
    idx = mix_index(index, N, student.device)
    stem = _by_k("softmax_mixmse", K)
    nbytes = getattr(_lib.load(), f"{stem}_ws_bytes")(N, H * W)
    ws = _ws(nbytes, student.device)
    loss = _f32(1, student.device)
    _lib.call(f"{stem}_fwd", student.data_ptr(), teacher.data_ptr(), idx.data_ptr(), float(w_self), float(w_other),
              loss.data_ptr(), N, H * W, K, ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_mixmse_bwd(student: Tensor, teacher: Tensor, index: Tensor, w_self: float, w_other: float,
                       gscale: Tensor) -> Tensor:
    """the student's gradient (the teacher carries none)"""
    N, K, H, W = student.shape
    idx = mix_index(index, N, student.device)
    d = empty_nhwc(N, K, H, W, torch.float32, student.device)
    _lib.call(_by_k("softmax_mixmse", K) + "_bwd", student.data_ptr(), teacher.data_ptr(), idx.data_ptr(),
              float(w_self), float(w_other), gscale.data_ptr(), d.data_ptr(), N, H * W, K, _stream())
    return d


# --------------------------------------------------------------------------- DAE prior, orthogonal prototypes (csrc/cy_prior.hip)
PRIOR_FORMS = {"dae": _lib.CY_PRIOR_DAE, "ortho": _lib.CY_PRIOR_ORTHO}
PRIOR_ACTS = {"sigmoid": _lib.CY_PRIOR_ACT_SIGMOID, "tanh": _lib.CY_PRIOR_ACT_TANH}


def prior_plan(form: str, K: int, Cc: int, npix: int = 0, align: int = 16) -> dict:
    """the launch rule of the DAE ("dae": K classes, Cc image channels, npix pixels, the logits' base aligned to `align`
    bytes) and orthogonality ("ortho": K prototypes of Cc floats) kernels: the values of cy_prior_plan by name.  A
    host-side query, no GPU needed; what the launches refuse raises HipKernelError with their status."""
    return _query(_lib.PriorPlan, "cy_prior_plan", PRIOR_FORMS[form], int(npix), int(K), int(Cc), int(align))


def _dae_args(logits: Tensor, weight: Tensor, bias: Tensor, image: Tensor):
    N, K, H, W = logits.shape
    assert image.dim() == 4 and image.shape[0] == N and tuple(image.shape[2:]) == (H, W), \
        (tuple(image.shape), tuple(logits.shape))
    assert weight.numel() == K and bias.numel() == 1, (tuple(weight.shape), tuple(bias.shape), K)
    assert image.dtype == torch.float32 and image.is_contiguous(), (image.dtype, image.stride())
    return N, K, H * W, image.shape[1]


def dae_fwd(logits: Tensor, weight: Tensor, bias: Tensor, image: Tensor, act: int) -> Tensor:
    """logits f32 [N,K,H,W] with NHWC memory, weight f32 [K] (any shape of K elements), bias f32 [1], image f32
    [N,Cimg,H,W] contiguous -> device scalar: F.mse_loss(act(conv1x1(logits)), image)"""
    N, K, HW, Cimg = _dae_args(logits, weight, bias, image)
    nbytes = _lib.load().cy_dae_ws_bytes(N * HW, K, 0)
    ws = _ws(nbytes, logits.device)
    loss = _f32(1, logits.device)
    _lib.call("cy_dae_fwd", logits.data_ptr(), weight.data_ptr(), bias.data_ptr(), image.data_ptr(), loss.data_ptr(),
              N, HW, K, Cimg, int(act), ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def dae_bwd(logits: Tensor, weight: Tensor, bias: Tensor, image: Tensor, act: int, gscale: Tensor):
    """-> (dlogits [N,K,H,W] with NHWC memory, dweight [K], dbias [1])"""
    N, K, HW, Cimg = _dae_args(logits, weight, bias, image)
    nbytes = _lib.load().cy_dae_ws_bytes(N * HW, K, 1)
    ws = _ws(nbytes, logits.device)
    d = empty_nhwc(N, K, logits.shape[2], logits.shape[3], torch.float32, logits.device)
    dw, db = _f32(K, logits.device), _f32(1, logits.device)
    _lib.call("cy_dae_bwd", logits.data_ptr(), weight.data_ptr(), bias.data_ptr(), image.data_ptr(), gscale.data_ptr(),
              d.data_ptr(), dw.data_ptr(), db.data_ptr(), N, HW, K, Cimg, int(act), ws.data_ptr(), nbytes, _stream())
    return d, dw, db


def ortho_fwd(prototypes: Tensor) -> Tensor:
    """prototypes f32 [K, C] contiguous -> device scalar: ((n n^T - I)^2).mean() of the normalised rows"""
    K, Cc = prototypes.shape
    loss = _f32(1, prototypes.device)
    _lib.call("cy_ortho_fwd", prototypes.data_ptr(), loss.data_ptr(), K, Cc, _stream())
    return loss.view(())


def ortho_bwd(prototypes: Tensor, gscale: Tensor) -> Tensor:
    K, Cc = prototypes.shape
    d = _f32(K * Cc, prototypes.device).view(K, Cc)
    _lib.call("cy_ortho_bwd", prototypes.data_ptr(), gscale.data_ptr(), d.data_ptr(), K, Cc, _stream())
    return d


# --------------------------------------------------------------------------- differentiable mean teacher (csrc/cy_teacher.hip)
TEACHER_FORMS = {"adam": _lib.CY_TEACHER_ADAM, "axpy": _lib.CY_TEACHER_AXPY, "ema_multi": _lib.CY_TEACHER_EMA_MULTI,
                 "gathermse": _lib.CY_TEACHER_GATHERMSE}
EMA_MULTI_MAX = 4096  # tensors of one cy_ema_update_multi launch
SOURCE_MAP_MAX = 1 << 24  # pixel indices an f32 image carries exactly


def teacher_plan(form: str, n: int, K: int = 0, align: int = 16) -> dict:
    """the launch rule of the teacher kernels (host-side query, no GPU needed): the values of cy_teacher_plan by name.
    `n`: elements ("adam", "axpy"), tensors ("ema_multi") or pixels ("gathermse").  What the launches refuse raises
    HipKernelError with their status."""
    return _query(_lib.TeacherPlan, "cy_teacher_plan", TEACHER_FORMS[form], int(n), int(K), int(align))


def _flat_f32(*ts: Tensor) -> int:
    require_gpu(*ts)
    n = ts[0].numel()
    for t in ts:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, (t.dtype, t.stride(), t.numel(), n)
    return n


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float, eps: float,
              wd: float, step: int) -> None:
    """one torch.optim.Adam update (amsgrad=False, maximize=False) of flat f32 buffers, in place; `step` is the 1-based
    count after this update"""
    n = _flat_f32(p, g, m, v)
    _lib.call("cy_adam_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(lr), float(beta1),
              float(beta2), float(eps), float(wd), int(step), _stream())


def axpy(y: Tensor, x: Tensor, a: float) -> None:
    """y += a * x over flat f32 buffers, in place"""
    n = _flat_f32(y, x)
    _lib.call("cy_axpy", y.data_ptr(), x.data_ptr(), n, float(a), _stream())


# --------------------------------------------------------------------------- SGD / Adam / AdamW on flat buffers (csrc/cy_optim.hip)
OPTIM_FORMS = {"sgd": _lib.CY_OPTIM_SGD, "adamw": _lib.CY_OPTIM_ADAMW}


def optim_plan(form: str, n: int, align: int = 16) -> dict:
    """the launch rule of cy_sgd_step / cy_adamw_step (host-side query, no GPU needed): the values of cy_optim_plan by
    name -- the rule teacher_plan("adam", ...) gives.  What the launches refuse raises HipKernelError with their
    status."""
    return _query(_lib.OptimPlan, "cy_optim_plan", OPTIM_FORMS[form], int(n), int(align))


def sgd_step(p: Tensor, g: Tensor, buf: Optional[Tensor], lr: float, momentum: float, dampening: float, wd: float,
             nesterov: bool, first: bool) -> None:
    """one torch.optim.SGD update (maximize=False) of flat f32 buffers, in place; `buf` is None exactly when
    momentum == 0; `first`: this is the update that copies the gradient into the momentum buffer"""
    n = _flat_f32(p, g) if buf is None else _flat_f32(p, g, buf)
    _lib.call("cy_sgd_step", p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), n, float(lr),
              float(momentum), float(dampening), float(wd), int(bool(nesterov)), int(bool(first)), _stream())


def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, vmax: Optional[Tensor], lr: float, beta1: float,
               beta2: float, eps: float, wd: float, decoupled: bool, step: int) -> None:
    """one torch.optim.AdamW (`decoupled`) or torch.optim.Adam update (maximize=False) of flat f32 buffers, in place;
    a `vmax` buffer is amsgrad; `step` is the 1-based count after this update"""
    n = _flat_f32(p, g, m, v) if vmax is None else _flat_f32(p, g, m, v, vmax)
    _lib.call("cy_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
              None if vmax is None else vmax.data_ptr(), n, float(lr), float(beta1), float(beta2), float(eps),
              float(wd), int(bool(decoupled)), int(step), _stream())


def ema_table(pairs, device) -> Tensor:
    """the int64 [count, 3] device table of cy_ema_update_multi for (teacher, student) f32 tensor pairs: the two
    addresses and the element count of each.  Built on the host and uploaded once; the caller caches it and rebuilds
    it when an address changed."""
    rows = []
    for t, s in pairs:
        require_gpu(t, s)
        assert t.dtype == s.dtype == torch.float32 and t.is_contiguous() and s.is_contiguous(), (t.dtype, s.dtype)
        assert t.numel() == s.numel(), (tuple(t.shape), tuple(s.shape))
        rows.append((t.data_ptr(), s.data_ptr(), t.numel()))
    if not 1 <= len(rows) <= EMA_MULTI_MAX:
        raise ValueError(f"a multi-tensor EMA launch covers 1..{EMA_MULTI_MAX} tensors, got {len(rows)}")
    return torch.tensor(rows, dtype=torch.int64).to(device)


def ema_update_multi(table: Tensor, alpha: float, weight_decay: float) -> None:
    """the update of `ema_update` over every (teacher, student, n) row of an `ema_table`, in one launch"""
    require_gpu(table)
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 3 and table.is_contiguous()
    _lib.call("cy_ema_update_multi", table.data_ptr(), table.shape[0], float(alpha), float(weight_decay), _stream())


def source_map_from_warped(warped_index: Tensor) -> Tensor:
    """int32 [N,H,W] source map of the gather-MSE kernels from what the step's nearest-neighbour warp made of an
    [N,1,H,W] f32 image holding `pixel index + 1` (ops.source_index_image): the source pixel, or -1 where the warp
    padded with zero"""
    N, Cc, H, W = warped_index.shape
    assert Cc == 1 and warped_index.dtype == torch.float32, (tuple(warped_index.shape), warped_index.dtype)
    return (warped_index.reshape(N, H, W).to(torch.int32) - 1).contiguous()


def source_index_image(N: int, H: int, W: int, device) -> Tensor:
    """[N,1,H,W] f32, every image holding 1 .. H*W in row-major order: exact in f32 below 2^24 pixels"""
    assert H * W < SOURCE_MAP_MAX, f"an f32 image carries pixel indices exactly below 2^24 pixels, got {H}x{W}"
    one = torch.arange(1, H * W + 1, dtype=torch.float32, device=device).view(1, 1, H, W)
    return one.expand(N, 1, H, W).contiguous()


def _gather_args(teacher: Tensor, source_map: Tensor, student: Tensor):
    N, K, H, W = student.shape
    assert teacher.shape == student.shape, (tuple(teacher.shape), tuple(student.shape))
    assert teacher.dtype == student.dtype == torch.float32 and is_nhwc(teacher) and is_nhwc(student)
    assert source_map.dtype == torch.int32 and source_map.numel() == N * H * W and source_map.is_contiguous(), \
        (source_map.dtype, tuple(source_map.shape))
    return N, K, H * W


def softmax_gathermse_fwd(teacher: Tensor, source_map: Tensor, student: Tensor) -> Tensor:
    """teacher (unwarped), student: f32 logits [N,K,H,W] with NHWC memory; source_map int32 [N,H,W] (the source pixel of
    the same image, or -1) -> device scalar: the mean of (q - softmax(student))^2, q the teacher's softmax at the
    source or 0 outside"""
    N, K, HW = _gather_args(teacher, source_map, student)
    nbytes = _lib.load().cy_softmax_gathermse_ws_bytes(N, HW)
    ws = _ws(nbytes, student.device)
    loss = _f32(1, student.device)
    _lib.call("cy_softmax_gathermse_fwd", teacher.data_ptr(), source_map.data_ptr(), student.data_ptr(),
              loss.data_ptr(), N, HW, K, ws.data_ptr(), nbytes, _stream())
    return loss.view(())


def softmax_gathermse_bwd(teacher: Tensor, source_map: Tensor, student: Tensor, gscale: Tensor) -> Tensor:
    """the student's gradient (the teacher side carries none)"""
    N, K, HW = _gather_args(teacher, source_map, student)
    d = empty_nhwc(N, K, student.shape[2], student.shape[3], torch.float32, student.device)
    _lib.call("cy_softmax_gathermse_bwd", teacher.data_ptr(), source_map.data_ptr(), student.data_ptr(),
              gscale.data_ptr(), d.data_ptr(), N, HW, K, _stream())
    return d


def dice_counts(logits: Tensor, target: Tensor) -> Tensor:
    """int64 [N,K,2] = per-sample per-class (intersection, union) of argmax(logits) vs target."""
    N, K, H, W = logits.shape
    counts = torch.empty((N, K, 2), dtype=torch.int64, device=logits.device)
    _lib.call("cy_dice_counts", logits.data_ptr(), target.data_ptr(), counts.data_ptr(), N, H * W, K,
              _stream())
    return counts


def group_dice_counts(logits: Tensor, target: Tensor, G: int) -> Tensor:
    """int64 [N,G,2] = per-sample per-class (intersection, union) of the arg-max over the G group sums of
    softmax(logits) (K/G contiguous channels per class) vs target."""
    N, K, H, W = logits.shape
    counts = torch.empty((N, int(G), 2), dtype=torch.int64, device=logits.device)
    _lib.call("cy_group_dice_counts", logits.data_ptr(), target.data_ptr(), counts.data_ptr(), N, H * W, K, int(G),
              _stream())
    return counts


def mix_dice_counts(logits: Tensor, target: Tensor, mix: Tensor) -> Tensor:
    """int64 [N,C,2] = per-sample per-class (intersection, union) of the arg-max over softmax(logits) @ mix ([K, C])
    vs target."""
    N, K, H, W = logits.shape
    mix = _mix_arg(logits, mix)
    C = mix.shape[1]
    counts = torch.empty((N, C, 2), dtype=torch.int64, device=logits.device)
    _lib.call("cy_mix_dice_counts", logits.data_ptr(), target.data_ptr(), mix.data_ptr(), counts.data_ptr(), N, H * W,
              K, C, _stream())
    return counts


def surface_stats(pred: Tensor, target: Tensor, classes, ndim: int = 3, maps: bool = False):
    """Surface-distance statistics of two class-index volumes (csrc/cy_surface.hip).  pred, target: int64 [D, H, W]
    (ndim=3) or [H, W] / [1, H, W] (ndim=2); classes: the R reported class indices.  Returns device tensors
    (count int64 [2, R], sum f64 [2, R], maxd2 int32 [2, R]) -- direction 0 is pred -> target, 1 target -> pred -- and
    with maps=True also (d2 int32 [2, R, D, H, W], border uint8 [2, R, D, H, W]).  No host sync."""
    require_gpu(pred, target)
    assert pred.shape == target.shape, f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}."
    assert pred.dtype == torch.int64 and target.dtype == torch.int64, "class-index volumes are int64"
    if pred.dim() == 2:
        pred, target = pred[None], target[None]
    assert pred.dim() == 3, f"a volume is [D, H, W] or [H, W], given {tuple(pred.shape)}"
    pred, target = pred.contiguous(), target.contiguous()
    D, H, W = pred.shape
    cls = (C.c_int32 * len(classes))(*[int(c) for c in classes])
    R, dev = len(classes), pred.device
    count = torch.empty((2, R), dtype=torch.int64, device=dev)
    total = torch.empty((2, R), dtype=torch.float64, device=dev)
    maxd2 = torch.empty((2, R), dtype=torch.int32, device=dev)
    d2 = torch.empty((2, R, D, H, W), dtype=torch.int32, device=dev) if maps else None
    border = torch.empty((2, R, D, H, W), dtype=torch.uint8, device=dev) if maps else None
    nbytes = _lib.load().cy_surface_ws_bytes(D, H, W)
    ws = _ws(nbytes, dev)
    _lib.call("cy_surface_stats", pred.data_ptr(), target.data_ptr(), cls, R, D, H, W, int(ndim), count.data_ptr(),
              total.data_ptr(), maxd2.data_ptr(), _ptr(d2), _ptr(border), ws.data_ptr(), nbytes, _stream())
    if maps:
        return count, total, maxd2, d2, border
    return count, total, maxd2


# --------------------------------------------------------------------------- SLIC superpixels (csrc/cy_slic.hip)
SLIC_PLAN_FIELDS = _fields(_lib.SlicPlan)
_SLIC_WS = {}  # (device, N, H, W, n_segments) -> workspace; the calls of one shape are ordered by the stream they share


def slic_plan(N: int, H: int, W: int, n_segments: int = 40, sigma: float = 5.0, compactness: float = 0.1,
              max_iter: int = 10) -> dict:
    """what cy_slic would do for these sizes: geometry (r, S, start, Ky, Kx, K, M, min_size), kernel form, grids and
    LDS per stage; `status` is the refusal (0: none), nothing is launched and no GPU is needed"""
    return _query(_lib.SlicPlan, "cy_slic_plan", int(N), int(H), int(W), int(n_segments), float(sigma),
                  float(compactness), int(max_iter), check=False)


def _slic_images(images: Tensor) -> Tensor:
    require_gpu(images)
    if images.dim() == 4:
        if images.shape[1] != 1:
            raise ValueError(f"superpixels are computed on single-channel images, given {tuple(images.shape)}")
        images = images[:, 0]
    if images.dim() != 3:
        raise ValueError(f"images are [N,1,H,W] or [N,H,W], given {tuple(images.shape)}")
    return images.detach().float().contiguous()


def _slic_ws(dev, N: int, H: int, W: int, n_segments: int):
    key = (dev, N, H, W, int(n_segments))
    hit = _SLIC_WS.get(key)
    if hit is None:
        nbytes = _lib.load().cy_slic_ws_bytes(N, H, W, int(n_segments))
        hit = _SLIC_WS[key] = (_ws(nbytes, dev), nbytes)
    return hit


def slic_blur_q(images: Tensor, sigma: float = 5.0) -> Tensor:
    """stage 1: Gaussian blur (reflect boundary) and 16-bit quantisation -> q int32 [N,H,W]"""
    x = _slic_images(images)
    N, H, W = x.shape
    q = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    ws = _ws(4 * N * H * W + 256, x.device)
    _lib.call("cy_slic_blur_q", x.data_ptr(), q.data_ptr(), N, H, W, float(sigma), ws.data_ptr(), ws.numel(),
              _stream())
    return q


def slic_cluster(q: Tensor, n_segments: int = 40, compactness: float = 0.1, max_iter: int = 10):
    """stage 2: windowed k-means on the quantised image -> (labels int32 [N,H,W], centres int32 [N,K,3] = cy, cx, cq)"""
    require_gpu(q)
    assert q.dtype == torch.int32 and q.dim() == 3, "q is int32 [N,H,W]"
    q = q.contiguous()
    N, H, W = q.shape
    K = max(slic_plan(N, H, W, n_segments, 0.0, compactness, max_iter)["K"], 1)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=q.device)
    centres = torch.empty((N, K, 3), dtype=torch.int32, device=q.device)
    ws, nbytes = _slic_ws(q.device, N, H, W, n_segments)
    _lib.call("cy_slic_cluster", q.data_ptr(), labels.data_ptr(), centres.data_ptr(), N, H, W, int(n_segments),
              float(compactness), int(max_iter), ws.data_ptr(), nbytes, _stream())
    return labels, centres


def slic_connect(labels: Tensor, n_segments: int = 40):
    """stage 3: 4-connected components of a label map, the small ones merged -> (ids uint8 [N,H,W], count int32 [N])"""
    require_gpu(labels)
    assert labels.dtype == torch.int32 and labels.dim() == 3, "labels are int32 [N,H,W]"
    labels = labels.contiguous()
    N, H, W = labels.shape
    ids = torch.empty((N, H, W), dtype=torch.uint8, device=labels.device)
    count = torch.empty((N,), dtype=torch.int32, device=labels.device)
    ws, nbytes = _slic_ws(labels.device, N, H, W, n_segments)
    _lib.call("cy_slic_connect", labels.data_ptr(), ids.data_ptr(), count.data_ptr(), N, H, W, int(n_segments),
              ws.data_ptr(), nbytes, _stream())
    return ids, count


def slic(images: Tensor, n_segments: int = 40, sigma: float = 5.0, compactness: float = 0.1, max_iter: int = 10):
    """SLIC superpixels of single-channel images in 0..1 ([N,1,H,W] or [N,H,W]; bf16 / f16 are converted) ->
    (ids uint8 [N,H,W], count int32 [N]).  All on the current stream, no host read; the workspace is kept per shape."""
    x = _slic_images(images)
    N, H, W = x.shape
    ids = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
    count = torch.empty((N,), dtype=torch.int32, device=x.device)
    ws, nbytes = _slic_ws(x.device, N, H, W, n_segments)
    _lib.call("cy_slic", x.data_ptr(), ids.data_ptr(), count.data_ptr(), N, H, W, int(n_segments), float(sigma),
              float(compactness), int(max_iter), ws.data_ptr(), nbytes, _stream())
    return ids, count


# --------------------------------------------------------------------------- loader augmentation (csrc/cy_augment.hip)
AUG_MAX_SIDE, AUG_MAX_OUT, AUG_MAX_VIEWS = _lib.CY_AUG_MAX_SIDE, _lib.CY_AUG_MAX_OUT, _lib.CY_AUG_MAX_VIEWS
AUG_IP_LEN, AUG_FP_LEN = _lib.CY_AUG_IP_LEN, _lib.CY_AUG_FP_LEN
AUG_BRIGHTNESS, AUG_CONTRAST = _lib.CY_AUG_BRIGHTNESS, _lib.CY_AUG_CONTRAST
AUG_PLAN_FIELDS = _fields(_lib.AugPlan)
_AUG_LUTS = {}  # device -> (ToTensor's table, the identity label table)


def augment_plan(views: int, out_h: int, out_w: int) -> dict:
    """what cy_aug_views would launch for these sizes: kernel form, both grids, the trips of the jitter block over a
    view, its LDS bytes, the scratch bytes; `status` is the refusal (0: none); nothing is launched, no GPU needed"""
    return _query(_lib.AugPlan, "cy_aug_plan", int(views), int(out_h), int(out_w), check=False)


def augment_luts(device):
    """(ToTensor's 256 values exactly as torch computes them, uint8 -> float -> / 255; the identity label table)"""
    hit = _AUG_LUTS.get(device)
    if hit is None:
        ramp = torch.arange(256, dtype=torch.uint8)
        hit = _AUG_LUTS[device] = (ramp.float().div(255).to(device), ramp.to(device))
    return hit


def augment_views(store_images: Tensor, store_labels: Optional[Tensor], table: Tensor, int_params: Tensor,
                  f64_params: Tensor, label_lut: Optional[Tensor], out_hw, *, labels: bool = True):
    """The views the records describe, cut from a resident store -> (images f32 [B,1,h,w] in 0..1, labels int64
    [B,1,h,w] or None with labels=False).

    store_images / store_labels: uint8 arenas on the GPU; table: int64 [S,3] = (byte offset, H, W) on the HOST, where
    the records are checked against it before anything is launched.  The device reads no table: the row of each
    view's slice is written into its record here (the OFF_LO, OFF_HI, SRC_H, SRC_W columns of a copy; the caller's
    tensor is left as it is).  int_params int32 [B, AUG_IP_LEN] and f64_params float64 [B, AUG_FP_LEN] are HOST tensors
    (the records of include/contrastyou_hip.h, as contrastyou.augment.device draws them); they go up through `pinned`,
    whose ring makes the host wait only once it is a ring's worth of uploads ahead of the device.  label_lut: uint8
    [256] on the GPU, None for the identity.  Two launches on the current stream."""
    for name, t, dt in (("table", table, torch.int64), ("int_params", int_params, torch.int32),
                        ("f64_params", f64_params, torch.float64)):
        if t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} is a contiguous host tensor of {dt}, given {t.dtype} on {t.device}")
    B = int_params.shape[0]
    if tuple(int_params.shape) != (B, AUG_IP_LEN) or tuple(f64_params.shape) != (B, AUG_FP_LEN):
        raise ValueError(f"one record per view: int_params [B,{AUG_IP_LEN}] and f64_params [B,{AUG_FP_LEN}], given "
                         f"{tuple(int_params.shape)} and {tuple(f64_params.shape)}")
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1:
        raise ValueError(f"table is [S,3] = (byte offset, H, W), given {tuple(table.shape)}")
    if store_images.dtype != torch.uint8 or store_images.dim() != 1 or (
            labels and (store_labels is None or store_labels.dtype != torch.uint8
                        or store_labels.shape != store_images.shape)):
        raise ValueError("the store is two flat uint8 arenas of one size")
    if label_lut is not None and (label_lut.dtype != torch.uint8 or label_lut.numel() != 256):
        raise ValueError("label_lut is uint8 [256]")
    require_gpu(store_images, store_labels if labels else None, label_lut)
    dev = store_images.device
    h, w = int(out_hw[0]), int(out_hw[1])
    tensor_lut, identity = augment_luts(dev)
    lut = identity if label_lut is None else label_lut
    _lib.check(augment_plan(B, h, w)["status"], "cy_aug_views")  # sizes it refuses are not allocated first
    # each record takes the table row of its slice along; an index outside the table keeps the row of the nearest
    # slice and is refused by the library, which checks SLICE itself
    rows = table[int_params[:, _lib.CY_AUG_IP_SLICE].long().clamp(0, table.shape[0] - 1)]
    int_params = int_params.clone()
    int_params[:, _lib.CY_AUG_IP_OFF_LO] = (rows[:, 0] & 0xffffffff).to(torch.int32)  # wraps to the low word's bits
    int_params[:, _lib.CY_AUG_IP_OFF_HI] = (rows[:, 0] >> 32).to(torch.int32)
    int_params[:, _lib.CY_AUG_IP_SRC_H] = rows[:, 1].to(torch.int32)
    int_params[:, _lib.CY_AUG_IP_SRC_W] = rows[:, 2].to(torch.int32)
    images = torch.empty((B, 1, h, w), dtype=torch.float32, device=dev)
    gts = torch.empty((B, 1, h, w), dtype=torch.int64, device=dev) if labels else None
    scratch = _ws(B * h * w, dev)
    ip_dev, fp_dev = pinned.upload(int_params, dev), pinned.upload(f64_params, dev)
    _lib.call("cy_aug_views", store_images.data_ptr(), store_labels.data_ptr() if labels else None, table.data_ptr(),
              table.shape[0], store_images.numel(), ip_dev.data_ptr(), int_params.data_ptr(), fp_dev.data_ptr(), B, h, w,
              lut.data_ptr(), tensor_lut.data_ptr(), images.data_ptr(), _ptr(gts), scratch.data_ptr(), scratch.numel(),
              _stream())
    return images, gts


# --------------------------------------------------------------------------- projector pieces
def avgpool_fwd(x: Tensor) -> Tensor:
    N, Cc, H, W = x.shape
    pooled = _f32(N * Cc, x.device).view(N, Cc)
    _lib.call("cy_avgpool_fwd", x.data_ptr(), pooled.data_ptr(), N, H * W, Cc, dtype_code(x.dtype),
              _stream())
    return pooled


def avgpool_bwd(dpooled: Tensor, shape, dtype) -> Tensor:
    N, Cc, H, W = shape
    dx = empty_nhwc(N, Cc, H, W, dtype, dpooled.device)
    _lib.call("cy_avgpool_bwd", dpooled.data_ptr(), dx.data_ptr(), N, H * W, Cc, dtype_code(dtype),
              _stream())
    return dx


def linear_fwd(x: Tensor, w: Tensor, b: Optional[Tensor], act: int = 0, slope: float = 0.01) -> Tensor:
    M, I = x.shape
    O = w.shape[0]
    y = _f32(M * O, x.device).view(M, O)
    _lib.call("cy_linear_fwd", x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), M, I, O, act,
              float(slope), _stream())
    return y


def linear_bwd(x: Tensor, w: Tensor, y: Tensor, dy: Tensor, act: int, slope: float, need_dx: bool,
               need_dw: bool, dw_into: Optional[Tensor] = None, db_into: Optional[Tensor] = None):
    """dx, dw, db; with dw_into / db_into the parameter gradients are ADDED into those buffers (returned as None)"""
    M, I = x.shape
    O = w.shape[0]
    dx = _f32(M * I, x.device).view(M, I) if need_dx else None
    if dw_into is not None:
        with ordered(("lin_grad", dw_into.data_ptr())):
            _lib.call("cy_linear_bwd_into", x.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr(), _ptr(dx),
                      dw_into.data_ptr(), _ptr(db_into), M, I, O, act, float(slope), _stream())
        return dx, None, None
    dw = _f32(O * I, x.device).view(O, I) if need_dw else None
    db = _f32(O, x.device) if need_dw else None
    _lib.call("cy_linear_bwd", x.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr(), _ptr(dx),
              _ptr(dw), _ptr(db), M, I, O, act, float(slope), _stream())
    return dx, dw, db


def proj_head_ok(x: Tensor, w1: Tensor, w2: Tensor) -> bool:
    """shapes the one-launch projection head takes (csrc/cy_proj_head.hip proj_head_*)"""
    Cc, hid, out = x.shape[1], w1.shape[0], w2.shape[0]
    return (x.is_cuda and Cc % 8 == 0 and Cc <= 512 and hid % 4 == 0 and hid <= 512 and out <= 512
            and x.dtype in (torch.bfloat16, torch.float16, torch.float32))


def proj_head_fwd(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, slope: float = 0.01,
                  eps: float = 1e-12):
    """x NHWC [B,C,H,W] -> z [B,out] normalised, and (pooled, y1, y2, norms) for the backward"""
    B, Cc, H, W = x.shape
    hid, out = w1.shape[0], w2.shape[0]
    dev = x.device
    pooled, y1 = _f32(B * Cc, dev).view(B, Cc), _f32(B * hid, dev).view(B, hid)
    y2, norms = _f32(B * out, dev).view(B, out), _f32(B, dev)
    z = torch.empty((B, out), dtype=torch.float32, device=dev)  # (not a view: SupConLoss1 rejoins its two chunks through z)
    _lib.call("cy_proj_head_fwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
              pooled.data_ptr(), y1.data_ptr(), y2.data_ptr(), z.data_ptr(), norms.data_ptr(), B, H * W, Cc, hid, out,
              float(slope), float(eps), dtype_code(x.dtype), _stream())
    return z, pooled, y1, y2, norms


def proj_head_bwd(dz: Tensor, pooled: Tensor, y1: Tensor, y2: Tensor, norms: Tensor, w1: Tensor, w2: Tensor, shape,
                  dtype, need_dx: bool, sinks=None, slope: float = 0.01, eps: float = 1e-12):
    """-> dx (NHWC, dtype) or None, and (dw1, db1, dw2, db2) -- None each when `sinks` (the parameters' .grad buffers,
    added into) is given"""
    B, Cc, H, W = shape
    hid, out = w1.shape[0], w2.shape[0]
    dev = dz.device
    dx = empty_nhwc(B, Cc, H, W, dtype, dev) if need_dx else None
    nbytes = _lib.load().cy_proj_head_bwd_ws_bytes(B, hid, out)
    ws = _ws(nbytes, dev)
    if sinks is not None:
        g = sinks
        acc = 1
    else:
        g = (_f32(hid * Cc, dev).view(hid, Cc), _f32(hid, dev), _f32(out * hid, dev).view(out, hid), _f32(out, dev))
        acc = 0

    def launch():
        _lib.call("cy_proj_head_bwd", dz.data_ptr(), pooled.data_ptr(), y1.data_ptr(), y2.data_ptr(), norms.data_ptr(),
                  w1.data_ptr(), w2.data_ptr(), _ptr(dx), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                  g[3].data_ptr(), acc, ws.data_ptr(), nbytes, B, H * W, Cc, hid, out, float(slope), float(eps),
                  dtype_code(dtype), _stream())

    if sinks is not None:
        with ordered(("lin_grad", g[0].data_ptr())):
            launch()
        return dx, (None, None, None, None)
    launch()
    return dx, g


def l2norm_fwd(x: Tensor, eps: float = 1e-12):
    M, D = x.shape
    z = torch.empty_like(x)
    norms = _f32(M, x.device)
    _lib.call("cy_l2norm_fwd", x.data_ptr(), z.data_ptr(), norms.data_ptr(), M, D, float(eps), _stream())
    return z, norms


def l2norm_bwd(x: Tensor, norms: Tensor, dz: Tensor, eps: float = 1e-12) -> Tensor:
    M, D = x.shape
    dx = torch.empty_like(x)
    _lib.call("cy_l2norm_bwd", x.data_ptr(), norms.data_ptr(), dz.data_ptr(), dx.data_ptr(), M, D,
              float(eps), _stream())
    return dx


# --------------------------------------------------------------------------- SupCon / InfoNCE
def supcon_fwd(P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float):
    R, D = P.shape
    n = R // 2
    S = _f32(R * R, P.device).view(R, R)
    stats = _f32(R * 4, P.device).view(R, 4)
    loss = _f32(1, P.device)
    _lib.call("cy_supcon_fwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), S.data_ptr(),
              loss.data_ptr(), stats.data_ptr(), n, D, float(t), _stream())
    return loss.view(()), S, stats


def supcon_bwd(P: Tensor, labels, pos_mask, S: Tensor, stats: Tensor, gscale: Tensor, t: float) -> Tensor:
    R, D = P.shape
    G = _f32(R * R, P.device)
    dP = torch.empty_like(P)
    _lib.call("cy_supcon_bwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), S.data_ptr(),
              stats.data_ptr(), gscale.data_ptr(), G.data_ptr(), dP.data_ptr(), R // 2, D, float(t),
              _stream())
    return dP


def supcon_excl_fwd(P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float):
    """SupConLoss1(exclude_other_pos=True): (loss, S, row statistics, tmp) on the materialised similarity matrix"""
    R, D = P.shape
    S = _f32(R * R, P.device).view(R, R)
    stats = _f32(R * 4, P.device).view(R, 4)
    tmp = _f32(R * 4 + 1, P.device)
    loss = _f32(1, P.device)
    _lib.call("cy_supcon_excl_fwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), S.data_ptr(), loss.data_ptr(),
              stats.data_ptr(), tmp.data_ptr(), R // 2, D, float(t), _stream())
    return loss.view(()), S, stats, tmp


def supcon_excl_bwd(P: Tensor, labels, pos_mask, S: Tensor, stats: Tensor, tmp: Tensor, gscale: Tensor, t: float) -> Tensor:
    R, D = P.shape
    G = _f32(R * R, P.device)
    dP = torch.empty_like(P)
    _lib.call("cy_supcon_excl_bwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), S.data_ptr(), stats.data_ptr(),
              tmp.data_ptr(), gscale.data_ptr(), G.data_ptr(), dP.data_ptr(), R // 2, D, float(t), _stream())
    return dP


SUPCON_FUSED = os.environ.get("CY_SUPCON_FUSED", "1") != "0"


def supcon_fused_ok(P: Tensor) -> bool:
    return SUPCON_FUSED and P.shape[1] <= 256 and P.shape[1] % 8 == 0


def supcon_fwd_fused(P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float):
    """loss, diag(S), row statistics; the similarity matrix is never materialised (csrc/cy_contrast.hip)"""
    R, D = P.shape
    n = R // 2
    nbytes = _lib.load().cy_supcon_fused_ws_bytes(n, D)
    ws = _ws(nbytes, P.device)
    stats = _f32(R * 4, P.device).view(R, 4)
    diag = _f32(R, P.device)
    loss = _f32(1, P.device)
    _lib.call("cy_supcon_fused_fwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), loss.data_ptr(), stats.data_ptr(),
              diag.data_ptr(), ws.data_ptr(), nbytes, n, D, float(t), _stream())
    return loss.view(()), diag, stats


def supcon_bwd_fused(P: Tensor, labels, pos_mask, stats: Tensor, gscale: Tensor, t: float) -> Tensor:
    R, D = P.shape
    nbytes = _lib.load().cy_supcon_fused_ws_bytes(R // 2, D)
    ws = _ws(nbytes, P.device)
    dP = torch.empty_like(P)
    _lib.call("cy_supcon_fused_bwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), stats.data_ptr(), gscale.data_ptr(),
              dP.data_ptr(), ws.data_ptr(), nbytes, R // 2, D, float(t), _stream())
    return dP


def supcon_sp_fwd(P: Tensor, labels: Optional[Tensor], pos_mask: Optional[Tensor], t: float, gamma: float, soft: bool,
                  correct_grad: bool):
    """SelfPacedSupConLoss on the fused kernels: aux = (loss, ratio, scale, sum of positive counts), diag(S), row
    statistics (D_i, c_i, W_i, M); the similarity matrix is never materialised (csrc/cy_contrast.hip)"""
    R, D = P.shape
    n = R // 2
    nbytes = _lib.load().cy_supcon_sp_ws_bytes(n, D)
    ws = _ws(nbytes, P.device)
    stats = _f32(R * 4, P.device).view(R, 4)
    diag = _f32(R, P.device)
    aux = _f32(4, P.device)
    _lib.call("cy_supcon_sp_fwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), aux.data_ptr(), stats.data_ptr(),
              diag.data_ptr(), ws.data_ptr(), nbytes, n, D, float(t), float(gamma), int(bool(soft)),
              int(bool(correct_grad)), _stream())
    return aux, diag, stats


def supcon_sp_bwd(P: Tensor, labels, pos_mask, stats: Tensor, aux: Tensor, gscale: Tensor, t: float, gamma: float,
                  soft: bool) -> Tensor:
    R, D = P.shape
    nbytes = _lib.load().cy_supcon_sp_ws_bytes(R // 2, D)
    ws = _ws(nbytes, P.device)
    dP = torch.empty_like(P)
    _lib.call("cy_supcon_sp_bwd", P.data_ptr(), _ptr(labels), _ptr(pos_mask), stats.data_ptr(), aux.data_ptr(),
              gscale.data_ptr(), dP.data_ptr(), ws.data_ptr(), nbytes, R // 2, D, float(t), float(gamma),
              int(bool(soft)), _stream())
    return dP


def supcon_matrices(S: Tensor, stats: Tensor, labels, pos_mask):
    R = S.shape[0]
    outs = [_f32(R * R, S.device).view(R, R) for _ in range(4)]
    _lib.call("cy_supcon_matrices", S.data_ptr(), stats.data_ptr(), _ptr(labels), _ptr(pos_mask),
              *[o.data_ptr() for o in outs], R // 2, _stream())
    return outs  # sim_logits, sim_exp, pos_mask, neg_mask


def sgemm(A: Tensor, B: Tensor, alpha: float = 1.0, b_trans: bool = False) -> Tensor:
    M, K = A.shape
    N = B.shape[0] if b_trans else B.shape[1]
    Cm = _f32(M * N, A.device).view(M, N)
    _lib.call("cy_sgemm", A.data_ptr(), B.data_ptr(), Cm.data_ptr(), M, N, K, float(alpha),
              int(b_trans), _stream())
    return Cm


# --------------------------------------------------------------------------- affine / EMA / RAdam
def affine_fwd(x: Tensor, theta: Tensor, gamma: Optional[Tensor] = None) -> Tensor:
    require_gpu(x, theta)
    x = to_nhwc(x)
    N, Cc, H, W = x.shape
    out = empty_nhwc(N, Cc, H, W, x.dtype, x.device)
    _lib.call("cy_affine_nearest_fwd", x.data_ptr(), out.data_ptr(), theta.data_ptr(), _ptr(gamma), N,
              Cc, H, W, dtype_code(x.dtype), _stream())
    return out


def affine_bwd(dout: Tensor, theta: Tensor) -> Tensor:
    dout = to_nhwc(dout)
    N, Cc, H, W = dout.shape
    dx = empty_nhwc(N, Cc, H, W, dout.dtype, dout.device)
    _lib.call("cy_affine_nearest_bwd", dout.data_ptr(), dx.data_ptr(), theta.data_ptr(), N, Cc, H, W,
              dtype_code(dout.dtype), _stream())
    return dx


def ema_update(teacher: Tensor, student: Tensor, alpha: float, weight_decay: float) -> None:
    require_gpu(teacher, student)
    _lib.call("cy_ema_update", teacher.data_ptr(), student.data_ptr(), teacher.numel(), float(alpha),
              float(weight_decay), _stream())


def radam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float,
               eps: float, wd: float, step: int) -> None:
    require_gpu(p, g)
    _lib.call("cy_radam_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
              float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step), _stream())


# --------------------------------------------------------------------------- dense projector / sampling
def _bins_tensor(bins, device) -> Optional[Tensor]:
    """host list/array of (image, bin row, bin col) -> int32 device tensor [nb,3] (sync-free upload)"""
    if bins is None:
        return None
    if isinstance(bins, Tensor):
        return bins if bins.is_cuda else pinned.upload(bins.to(torch.int32).contiguous(), device)
    return pinned.upload(torch.as_tensor(bins, dtype=torch.int32).reshape(-1, 3).contiguous(), device)


def dense_proj_plan(C_in: int, hid: int, dtype: torch.dtype = torch.bfloat16, slope: float = 0.01) -> dict:
    """which kernels cy_dense_proj_fwd / _bwd run for this map (host-side query, no GPU needed): form is
    _lib.CY_DENSE_PROJ_VALU, _MFMA_REG (C = 32 / 64 / 128) or _MFMA_STREAM (C = 256 / 512)"""
    return _query(_lib.DenseProjPlan, "cy_dense_proj_plan", int(C_in), int(hid), dtype_code(dtype), float(slope))


def dense_proj_fwd(x: Tensor, w1: Tensor, b1: Tensor, size: Tuple[int, int], bins: Optional[Tensor],
                   slope: float = 0.01) -> Tensor:
    """x NHWC [N,C,H,W]; w1 f32 [hid,C]; -> hpool f32 [nb, hid] = mean over each bin of lrelu(w1 x + b1)"""
    require_gpu(x, w1, b1)
    N, Cc, H, W = x.shape
    hid = w1.shape[0]
    nb = N * size[0] * size[1] if bins is None else bins.shape[0]
    out = _f32(nb * hid, x.device).view(nb, hid)
    _lib.call("cy_dense_proj_fwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), _ptr(bins), nb,
              out.data_ptr(), N, H, W, Cc, Cc, hid, size[0], size[1], slope, dtype_code(x.dtype), _stream())
    return out


def dense_proj_bwd(x: Tensor, w1: Tensor, b1: Tensor, size: Tuple[int, int], bins: Optional[Tensor],
                   dhpool: Tensor, need_dx: bool, need_dw: bool, slope: float = 0.01):
    N, Cc, H, W = x.shape
    hid = w1.shape[0]
    nb = dhpool.shape[0]
    dx = None
    if need_dx:
        dx = torch.zeros((N, H, W, Cc), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    dw = _f32(hid * Cc, x.device).view(hid, Cc) if need_dw else None
    db = _f32(hid, x.device) if need_dw else None
    nbytes = _lib.load().cy_dense_proj_bwd_ws_bytes(nb, Cc, hid)
    ws = _ws(nbytes, x.device)
    _lib.call("cy_dense_proj_bwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), _ptr(bins), nb,
              dhpool.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db), 0, N, H, W, Cc, Cc, hid, size[0], size[1],
              slope, dtype_code(x.dtype), ws.data_ptr(), nbytes, _stream())
    return dx, dw, db


def adaptive_avgpool_fwd(x: Tensor, size: Tuple[int, int], bins: Optional[Tensor] = None) -> Tensor:
    require_gpu(x)
    N, Cc, H, W = x.shape
    nb = N * size[0] * size[1] if bins is None else bins.shape[0]
    out = _f32(nb * Cc, x.device).view(nb, Cc)
    _lib.call("cy_adaptive_avgpool_fwd", x.data_ptr(), _ptr(bins), nb, out.data_ptr(), N, H, W, Cc, Cc,
              size[0], size[1], dtype_code(x.dtype), _stream())
    return out


def adaptive_avgpool_bwd(dpool: Tensor, shape, dtype, size: Tuple[int, int]) -> Tensor:
    N, Cc, H, W = shape
    dx = empty_nhwc(N, Cc, H, W, dtype, dpool.device)
    _lib.call("cy_adaptive_avgpool_bwd", dpool.data_ptr(), dx.data_ptr(), N, H, W, Cc, Cc, size[0], size[1],
              dtype_code(dtype), _stream())
    return dx


def adaptive_maxpool_fwd(x: Tensor, size: Tuple[int, int]):
    """nn.AdaptiveMaxPool2d(size) on an NHWC map -> (rows [N*sh*sw, C] f32, arg-max pixel indices int32)"""
    require_gpu(x)
    N, Cc, H, W = x.shape
    nb = N * size[0] * size[1]
    out = _f32(nb * Cc, x.device).view(nb, Cc)
    arg = torch.empty((nb, Cc), dtype=torch.int32, device=x.device)
    _lib.call("cy_adaptive_maxpool_fwd", x.data_ptr(), out.data_ptr(), arg.data_ptr(), N, H, W, Cc, Cc, size[0], size[1],
              dtype_code(x.dtype), _stream())
    return out, arg


def adaptive_maxpool_bwd(dpool: Tensor, arg: Tensor, shape, dtype, size: Tuple[int, int]) -> Tensor:
    N, Cc, H, W = shape
    dx = empty_nhwc(N, Cc, H, W, dtype, dpool.device)
    _lib.call("cy_adaptive_maxpool_bwd", dpool.data_ptr(), arg.data_ptr(), dx.data_ptr(), N, H, W, Cc, Cc, size[0],
              size[1], dtype_code(dtype), _stream())
    return dx


def gather_rows_fwd(src: Tensor, idx: Tensor) -> Tensor:
    require_gpu(src, idx)
    M, D = idx.shape[0], src.shape[1]
    out = _f32(M * D, src.device).view(M, D)
    _lib.call("cy_gather_rows_fwd", src.data_ptr(), idx.data_ptr(), out.data_ptr(), M, D, _stream())
    return out


def gather_rows_bwd(dout: Tensor, idx: Tensor, rows: int) -> Tensor:
    M, D = dout.shape
    dsrc = torch.zeros((rows, D), dtype=torch.float32, device=dout.device)
    _lib.call("cy_gather_rows_bwd", dout.data_ptr(), idx.data_ptr(), dsrc.data_ptr(), M, D, _stream())
    return dsrc


# --------------------------------------------------------------------------- per-row projector (csrc/cy_pixel_mlp.hip)
def pixel_mlp_ok(C_in: int, hid: int, out: int) -> bool:
    """the fused range of cy_pixel_mlp_* (hid == 0: the linear head)"""
    return 1 <= C_in <= 256 and 0 <= hid <= 256 and 1 <= out <= 256


def pixel_mlp_plan(M: int, C_in: int, hid: int, out: int, dtype: torch.dtype = torch.float32) -> dict:
    """the launch shape of cy_pixel_mlp_fwd / _bwd (host-side query, no GPU needed)"""
    return _query(_lib.PixelMlpPlan, "cy_pixel_mlp_plan", int(M), int(C_in), int(hid), int(out), dtype_code(dtype))


def _pixel_rows(x: Tensor) -> Tuple[int, int]:
    """(channels, pixel pitch in elements) of rows [R, C] whose channels are contiguous"""
    assert x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1], (x.shape, x.stride())
    return x.shape[1], x.stride(0)


def pixel_mlp_fwd(x: Tensor, idx: Optional[Tensor], w1: Tensor, b1: Tensor, w2: Optional[Tensor],
                  b2: Optional[Tensor], slope: float, normalize: bool):
    """x: rows [R, C] (f32 / bf16 / f16, row pitch >= C); idx: int32 [M] distinct rows or None (all rows); w1 f32
    [hid, C] and w2 f32 [out, hid], or w1 f32 [out, C] alone (linear) -> (y f32 [M, out], inv f32 [M] or None)"""
    require_gpu(x, w1, b1)
    Cc, ldx = _pixel_rows(x)
    M = x.shape[0] if idx is None else idx.shape[0]
    hid, out = (0, w1.shape[0]) if w2 is None else (w1.shape[0], w2.shape[0])
    y = _f32(M * out, x.device).view(M, out)
    inv = _f32(M, x.device) if normalize else None
    _lib.call("cy_pixel_mlp_fwd", x.data_ptr(), _ptr(idx), w1.data_ptr(), b1.data_ptr(), _ptr(w2), _ptr(b2),
              y.data_ptr(), _ptr(inv), M, Cc, ldx, hid, out, float(slope), int(bool(normalize)), dtype_code(x.dtype),
              _stream())
    return y, inv


def pixel_mlp_bwd(x: Tensor, idx: Optional[Tensor], w1: Tensor, b1: Tensor, w2: Optional[Tensor], y: Tensor,
                  inv: Optional[Tensor], dy: Tensor, slope: float, normalize: bool, need_dx: bool, need_dw: bool):
    """-> (dx like x: zero outside the listed rows, or None; dw1, db1, dw2, db2 f32 or None)"""
    Cc, ldx = _pixel_rows(x)
    M, out = dy.shape
    hid = 0 if w2 is None else w1.shape[0]
    dx = None
    if need_dx:  # (the kernel accumulates into the listed rows)
        dx = torch.zeros(x.shape[0] * ldx, dtype=x.dtype, device=x.device).as_strided(x.shape, x.stride())
    dw1 = db1 = dw2 = db2 = ws = None
    nbytes = 0
    if need_dw:
        dw1, db1 = _f32(w1.numel(), x.device).view(w1.shape), _f32(w1.shape[0], x.device)
        if hid:
            dw2, db2 = _f32(w2.numel(), x.device).view(w2.shape), _f32(out, x.device)
        nbytes = _lib.load().cy_pixel_mlp_bwd_ws_bytes(M, Cc, hid, out, dtype_code(x.dtype))
        ws = _ws(nbytes, x.device)
    _lib.call("cy_pixel_mlp_bwd", x.data_ptr(), _ptr(idx), w1.data_ptr(), b1.data_ptr(), _ptr(w2), y.data_ptr(),
              _ptr(inv), dy.data_ptr(), _ptr(dx), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), 0, M, Cc, ldx, hid, out,
              float(slope), int(bool(normalize)), dtype_code(x.dtype), _ptr(ws), nbytes, _stream())
    return dx, dw1, db1, dw2, db2


# --------------------------------------------------------------------------- cluster heads / discrete MI
def cluster_head_ok(C: int, S: int, k: int) -> bool:
    return C in (32, 64) and S * k <= 128 and k <= 32


def cluster_head_plan(M: int, C_in: int, S: int, k: int) -> dict:
    """the launch shape of cy_cluster_head_fwd / _bwd (host-side query, no GPU needed): fwd_waves, fwd_grid, fwd_trips,
    bwd_grid, bwd_trips, slabs"""
    return _query(_lib.ClusterPlan, "cy_cluster_head_plan", int(M), int(C_in), int(S), int(k))


def cluster_head_fwd(x: Tensor, w: Tensor, b: Optional[Tensor], S: int, k: int, T: float = 1.0) -> Tensor:
    """x: [M, C] rows (an NHWC map flattened over pixels) -> probs f32 [S, M, k] (csrc/cy_cluster_head.hip)"""
    require_gpu(x, w)
    M, Cc = x.shape
    probs = _f32(S * M * k, x.device).view(S, M, k)
    _lib.call("cy_cluster_head_fwd", x.data_ptr(), w.data_ptr(), _ptr(b), probs.data_ptr(), M, Cc, S * k, S, k,
              1.0 / T, dtype_code(x.dtype), _stream())
    return probs


def cluster_head_bwd(x: Tensor, w: Tensor, probs: Tensor, dprobs: Tensor, T: float, need_dx: bool, need_dw: bool):
    S, M, k = probs.shape
    Cc = x.shape[1]
    dx = torch.empty_like(x) if need_dx else None
    dw = db = ws = None
    nbytes = 0
    if need_dw:
        dw, db = _f32(S * k * Cc, x.device).view(S * k, Cc), _f32(S * k, x.device)
        nbytes = _lib.load().cy_cluster_head_bwd_ws_bytes(M, Cc)
        ws = _ws(nbytes, x.device)
    _lib.call("cy_cluster_head_bwd", x.data_ptr(), w.data_ptr(), probs.data_ptr(), dprobs.data_ptr(), _ptr(dx),
              _ptr(dw), _ptr(db), M, Cc, S * k, S, k, 1.0 / T, dtype_code(x.dtype), _ptr(ws), nbytes, _stream())
    return dx, dw, db


def group_softmax_fwd(logits: Tensor, S: int, k: int, T: float = 1.0) -> Tensor:
    """logits f32 [M, S*k] -> probs f32 [S, M, k]"""
    require_gpu(logits)
    M = logits.shape[0]
    probs = _f32(S * M * k, logits.device).view(S, M, k)
    _lib.call("cy_group_softmax_fwd", logits.data_ptr(), probs.data_ptr(), M, S, k, 1.0 / T, _stream())
    return probs


def group_softmax_plan(M: int, S: int, k: int) -> dict:
    """the launch plan of cy_group_softmax_fwd / _bwd (host-side query, no GPU needed): the fields of
    cy_group_softmax_plan_t.  S*k > 255 raises HipKernelError (CY_ERR_SHAPE), as both launches do."""
    return _query(_lib.GroupSoftmaxPlan, "cy_group_softmax_plan", int(M), int(S), int(k))


def group_softmax_bwd(probs: Tensor, dprobs: Tensor, T: float = 1.0) -> Tensor:
    S, M, k = probs.shape
    dl = _f32(M * S * k, probs.device).view(M, S * k)
    _lib.call("cy_group_softmax_bwd", probs.data_ptr(), dprobs.data_ptr(), dl.data_ptr(), M, S, k, 1.0 / T,
              _stream())
    return dl


def joint_plan(N: int, H: int, W: int, k: int, pad: int) -> dict:
    """the launch plan of cy_joint_fwd / _bwd for two [N,H,W,k] maps and padding `pad` (host-side query, no GPU needed):
    the fields of cy_joint_plan_t, and "ws_bytes", the forward's workspace.  Shapes the kernels refuse raise
    HipKernelError (CY_ERR_SHAPE)."""
    out = _query(_lib.JointPlan, "cy_joint_plan", int(N), int(H), int(W), int(k), int(pad))
    out["ws_bytes"] = int(_lib.load().cy_joint_ws_bytes(int(N), int(H), int(W), int(k), int(pad)))
    return out


def joint_fwd(x1: Tensor, x2: Tensor, N: int, H: int, W: int, k: int, pad: int, normalise: bool) -> Tensor:
    """x1, x2: f32 NHWC-contiguous [N,H,W,k] buffers -> J f32 [T*T, k, k]"""
    require_gpu(x1, x2)
    T = 2 * pad + 1
    J = _f32(T * T * k * k, x1.device).view(T * T, k, k)
    nbytes = _lib.load().cy_joint_ws_bytes(N, H, W, k, pad)
    ws = _ws(nbytes, x1.device)
    _lib.call("cy_joint_fwd", x1.data_ptr(), x2.data_ptr(), J.data_ptr(), N, H, W, k, pad, int(normalise),
              ws.data_ptr(), nbytes, _stream())
    return J


def joint_bwd(x1: Tensor, x2: Tensor, dJ: Tensor, gscale: Tensor, N: int, H: int, W: int, k: int, pad: int,
              normalise: bool, need1: bool, need2: bool):
    d1 = torch.empty_like(x1) if need1 else None
    d2 = torch.empty_like(x2) if need2 else None
    _lib.call("cy_joint_bwd", x1.data_ptr(), x2.data_ptr(), dJ.data_ptr(), gscale.data_ptr(), _ptr(d1), _ptr(d2),
              N, H, W, k, pad, int(normalise), _stream())
    return d1, d2


def iid_loss(J: Tensor, mode: int, symmetric: bool, lamda: float, eps: float, want_grad: bool = True):
    """-> (out2 [2] = loss(lamda), loss(1); P [TT,k,k] normalised joint; dJ or None)"""
    TT, k = J.shape[0], J.shape[1]
    out2 = _f32(2, J.device)
    P = torch.empty_like(J)
    dJ = torch.empty_like(J) if want_grad else None
    nbytes = _lib.load().cy_iid_loss_ws_bytes(TT, k)
    ws = _ws(nbytes, J.device)
    _lib.call("cy_iid_loss", J.data_ptr(), out2.data_ptr(), P.data_ptr(), _ptr(dJ), TT, k, mode, int(symmetric),
              lamda, eps, ws.data_ptr(), nbytes, _stream())
    return out2, P, dJ


JOINT_PATCH_KERNELS = {None: -1, "per_displacement": 0, "staged": 1}  # the forward kernel: the rule's choice, or forced


def joint_patch_plan(N: int, H: int, W: int, k: int, pad: int, patch: int, kernel: Optional[str] = None) -> dict:
    """the launch rule of the patch-wise joint kernels (host-side query, no GPU needed): the values of
    cy_joint_patch_plan by name, and "ws_bytes", the forward's workspace.  What the launches refuse raises
    HipKernelError with their status."""
    out = _query(_lib.JointPatchPlan, "cy_joint_patch_plan", int(N), int(H), int(W), int(k), int(pad), int(patch),
                 JOINT_PATCH_KERNELS[kernel])
    out["ws_bytes"] = int(_lib.load().cy_joint_patch_ws_bytes(int(N), int(H), int(W), int(k), int(pad), int(patch),
                                                              JOINT_PATCH_KERNELS[kernel]))
    return out


def joint_patch_fwd(x1: Tensor, x2: Tensor, pad: int, patch: int, normalise: bool, kernel: Optional[str] = None,
                    J: Optional[Tensor] = None) -> Tensor:
    """x1, x2: f32 NHWC-contiguous [N,H,W,k] buffers -> J f32 [P, T*T, k, k], the displaced joint of every patch of
    side `patch` (step patch // 2), zero-padded at the patch border; `J` may be given as a contiguous f32 view to write
    into, `kernel` forces a forward kernel (JOINT_PATCH_KERNELS)"""
    require_gpu(x1, x2)
    N, H, W, k = x1.shape
    assert x2.shape == x1.shape, (x1.shape, x2.shape)
    plan = joint_patch_plan(N, H, W, k, pad, patch, kernel)
    T = 2 * pad + 1
    J = _f32(plan["P"] * T * T * k * k, x1.device) if J is None else J
    ws = _ws(plan["ws_bytes"], x1.device)
    _lib.call("cy_joint_patch_fwd", x1.data_ptr(), x2.data_ptr(), J.data_ptr(), N, H, W, k, int(pad), int(patch),
              int(normalise), JOINT_PATCH_KERNELS[kernel], ws.data_ptr(), plan["ws_bytes"], _stream())
    return J.view(plan["P"], T * T, k, k)


def iid_patch_loss(J: Tensor, mode: int, lamda: float, eps: float, want_grad: bool = True, want_joint: bool = True,
                   out: Optional[Tuple[Tensor, ...]] = None):
    """J: f32 [P, TT, k, k] -> (loss [1] = mean of the patch losses, losses [P], Pj [P,TT,k,k] final joints or None,
    dJ [P,TT,k,k] = d loss / d J or None); `out` may give the four as contiguous f32 views to write into"""
    require_gpu(J)
    P, TT, k = J.shape[0], J.shape[1], J.shape[2]
    if out is None:
        out = (_f32(1, J.device), _f32(P, J.device), torch.empty_like(J) if want_joint else None,
               torch.empty_like(J) if want_grad else None)
    loss, losses, Pj, dJ = out
    nbytes = _lib.load().cy_iid_patch_loss_ws_bytes(P, TT, k)
    ws = _ws(nbytes, J.device)
    _lib.call("cy_iid_patch_loss", J.data_ptr(), loss.data_ptr(), losses.data_ptr(), _ptr(Pj), _ptr(dJ), P, TT, k,
              int(mode), float(lamda), float(eps), ws.data_ptr(), nbytes, _stream())
    return loss, losses, Pj, dJ


def joint_patch_bwd(x1: Tensor, x2: Tensor, dJ: Tensor, gscale: Tensor, pad: int, patch: int, normalise: bool,
                    need1: bool = True, need2: bool = True, d1: Optional[Tensor] = None, d2: Optional[Tensor] = None):
    """-> (dx1, dx2) [N,H,W,k] = gscale[0] * the adjoint of joint_patch_fwd applied to dJ; either may be skipped"""
    require_gpu(x1, x2, dJ, gscale)
    N, H, W, k = x1.shape
    d1 = (torch.empty_like(x1) if d1 is None else d1) if need1 else None
    d2 = (torch.empty_like(x2) if d2 is None else d2) if need2 else None
    _lib.call("cy_joint_patch_bwd", x1.data_ptr(), x2.data_ptr(), dJ.data_ptr(), gscale.data_ptr(), _ptr(d1), _ptr(d2),
              N, H, W, k, int(pad), int(patch), int(normalise), _stream())
    return d1, d2


# --------------------------------------------------------------------------- PICA, JSD, entropy prior
PICA_KMAX = 64  # classes of csrc/cy_pica.hip
JSD_MAPS = (2, 8)  # fewest and most maps of cy_jsd_*
REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def pui_loss(x: Tensor, y: Tensor, lamda: float, want_grad: bool = True):
    """x, y: f32 [N, K] contiguous rows -> (out [1], dJ [K,K] or None, coef [3,K]) of cy_pui_loss"""
    require_gpu(x, y)
    N, K = x.shape
    J = joint_fwd(x, y, N, 1, 1, K, 0, False)
    stats = _f32(3 * K, x.device)
    _lib.call("cy_pui_stats", x.data_ptr(), y.data_ptr(), stats.data_ptr(), N, K, _stream())
    out, coef = _f32(1, x.device), _f32(3 * K, x.device)
    dJ = torch.empty_like(J) if want_grad else None
    _lib.call("cy_pui_loss", J.data_ptr(), stats.data_ptr(), out.data_ptr(), _ptr(dJ), coef.data_ptr(), N, K,
              float(lamda), _stream())
    return out, dJ, coef.view(3, K)


def pui_loss_bwd(x: Tensor, y: Tensor, dJ: Tensor, coef: Tensor, g: Tensor, need_x: bool, need_y: bool):
    N, K = x.shape
    dx, dy = joint_bwd(x, y, dJ, g, N, 1, 1, K, 0, False, need_x, need_y)
    if need_x:
        _lib.call("cy_rows_axpb", x.data_ptr(), coef[0].data_ptr(), coef[2].data_ptr(), g.data_ptr(), dx.data_ptr(),
                  N, K, _stream())
    if need_y:
        _lib.call("cy_rows_axpb", y.data_ptr(), coef[1].data_ptr(), None, g.data_ptr(), dy.data_ptr(), N, K, _stream())
    return dx, dy


def puiseg_loss(x1: Tensor, x2: Tensor, pad: int, lamda: float, want_grad: bool = True):
    """x1, x2: f32 NHWC-contiguous [N,H,W,k] -> (out [1], dJ [T*T,k,k] or None) of cy_puiseg_loss"""
    require_gpu(x1, x2)
    N, H, W, k = x1.shape
    J = joint_fwd(x1, x2, N, H, W, k, pad, False)
    TT, M = J.shape[0], N * H * W
    out = _f32(1, x1.device)
    dJ = torch.empty_like(J) if want_grad else None
    nbytes = _lib.load().cy_puiseg_ws_bytes(M, TT, k)
    ws = _ws(nbytes, x1.device)
    _lib.call("cy_puiseg_loss", J.data_ptr(), x1.data_ptr(), out.data_ptr(), _ptr(dJ), TT, k, M, float(lamda),
              ws.data_ptr(), nbytes, _stream())
    return out, dJ


def puiseg_loss_bwd(x1: Tensor, x2: Tensor, dJ: Tensor, g: Tensor, pad: int, lamda: float, need1: bool, need2: bool):
    N, H, W, k = x1.shape
    d1, d2 = joint_bwd(x1, x2, dJ, g, N, H, W, k, pad, False, need1, need2)
    if need1:
        _lib.call("cy_puiseg_balance_bwd", x1.data_ptr(), g.data_ptr(), d1.data_ptr(), N * H * W, k, float(lamda),
                  _stream())
    return d1, d2


def _ptr_table(ts):
    return (C.c_void_p * len(ts))(*[_ptr(t) for t in ts])


def jsd_fwd(maps, R: int, Cc: int, S: int, reduction: str, eps: float) -> Tensor:
    """maps: 2..8 f32 buffers of one layout (cy_jsd_fwd) -> out [R] ("none") or [1]"""
    require_gpu(*maps)
    dev = maps[0].device
    out = _f32(R if reduction == "none" else 1, dev)
    nbytes = _lib.load().cy_stream_sum_ws_bytes(R)
    ws = _ws(nbytes, dev)
    _lib.call("cy_jsd_fwd", _ptr_table(maps), len(maps), out.data_ptr(), R, Cc, S, REDUCTIONS[reduction], float(eps),
              ws.data_ptr(), nbytes, _stream())
    return out


def jsd_bwd(maps, g: Tensor, needs, R: int, Cc: int, S: int, reduction: str, eps: float):
    """g: f32 [R] ("none") or [1] on the device -> the gradients of the maps asked for (None for the others)"""
    grads = [torch.empty_like(t) if need else None for t, need in zip(maps, needs)]
    _lib.call("cy_jsd_bwd", _ptr_table(maps), len(maps), g.data_ptr(), _ptr_table(grads), R, Cc, S,
              REDUCTIONS[reduction], float(eps), _stream())
    return grads


def entropy_prior_fwd(x: Tensor, prior: Optional[Tensor], eps: float) -> Tensor:
    """x: f32 [R, C] contiguous rows, prior f32 [C] or None (uniform) -> out [1] = log C - KL(prior, x)"""
    require_gpu(x, prior)
    R, Cc = x.shape
    out = _f32(1, x.device)
    nbytes = _lib.load().cy_stream_sum_ws_bytes(R)
    ws = _ws(nbytes, x.device)
    _lib.call("cy_entropy_prior_fwd", x.data_ptr(), _ptr(prior), out.data_ptr(), R, Cc, float(eps), ws.data_ptr(),
              nbytes, _stream())
    return out


def entropy_prior_bwd(x: Tensor, prior: Optional[Tensor], g: Tensor, eps: float) -> Tensor:
    R, Cc = x.shape
    dx = torch.empty_like(x)
    _lib.call("cy_entropy_prior_bwd", x.data_ptr(), _ptr(prior), g.data_ptr(), dx.data_ptr(), R, Cc, float(eps),
              _stream())
    return dx


# --------------------------------------------------------------------------- GroupNorm + SiLU, bilinear
def gn_silu_fwd(y: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, groups: int, eps: float):
    require_gpu(y, gamma, beta)
    N, Cc, H, W = y.shape
    out = empty_nhwc(N, Cc, H, W, y.dtype, y.device)
    mr = _f32(N * groups * 2, y.device)
    nbytes = _lib.load().cy_gn_ws_bytes(N, Cc)
    ws = _ws(nbytes, y.device)
    _lib.call("cy_gn_silu_fwd", y.data_ptr(), Cc, _ptr(bias), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
              Cc, mr.data_ptr(), N, H * W, Cc, groups, eps, dtype_code(y.dtype), ws.data_ptr(), nbytes, _stream())
    return out, mr


def gn_silu_bwd(y: Tensor, dz: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, mr: Tensor,
                groups: int):
    N, Cc, H, W = y.shape
    du = empty_nhwc(N, Cc, H, W, y.dtype, y.device)
    dg, dbt = _f32(Cc, y.device), _f32(Cc, y.device)
    dbias = _f32(Cc, y.device) if bias is not None else None
    nbytes = _lib.load().cy_gn_ws_bytes(N, Cc)
    ws = _ws(nbytes, y.device)
    _lib.call("cy_gn_silu_bwd", y.data_ptr(), Cc, dz.data_ptr(), Cc, _ptr(bias), gamma.data_ptr(), beta.data_ptr(),
              mr.data_ptr(), du.data_ptr(), Cc, dg.data_ptr(), dbt.data_ptr(), _ptr(dbias), 0, N, H * W, Cc, groups,
              dtype_code(y.dtype), ws.data_ptr(), nbytes, _stream())
    return du, dg, dbt, dbias


def gn_silu_mod_fwd(y: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, mod_s: Tensor, mod_t: Tensor,
                    groups: int, eps: float):
    """gn_silu_fwd with the time-embedding modulation (x * (scale + 1) + shift between the norm and SiLU,
    contrastyou/arch/unet2.py:216-220); mod_s / mod_t: f32 [N, C]"""
    require_gpu(y, gamma, beta, mod_s, mod_t)
    N, Cc, H, W = y.shape
    out = empty_nhwc(N, Cc, H, W, y.dtype, y.device)
    mr = _f32(N * groups * 2, y.device)
    nbytes = _lib.load().cy_gn_ws_bytes(N, Cc)
    ws = _ws(nbytes, y.device)
    _lib.call("cy_gn_silu_mod_fwd", y.data_ptr(), Cc, _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mod_s.data_ptr(),
              mod_t.data_ptr(), out.data_ptr(), Cc, mr.data_ptr(), N, H * W, Cc, groups, eps, dtype_code(y.dtype),
              ws.data_ptr(), nbytes, _stream())
    return out, mr


def gn_silu_mod_bwd(y: Tensor, dz: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, mod_s: Tensor,
                    mod_t: Tensor, mr: Tensor, groups: int):
    N, Cc, H, W = y.shape
    du = empty_nhwc(N, Cc, H, W, y.dtype, y.device)
    dg, dbt = _f32(Cc, y.device), _f32(Cc, y.device)
    dbias = _f32(Cc, y.device) if bias is not None else None
    dms, dmt = _f32(N * Cc, y.device).view(N, Cc), _f32(N * Cc, y.device).view(N, Cc)
    nbytes = _lib.load().cy_gn_ws_bytes(N, Cc)
    ws = _ws(nbytes, y.device)
    _lib.call("cy_gn_silu_mod_bwd", y.data_ptr(), Cc, dz.data_ptr(), Cc, _ptr(bias), gamma.data_ptr(), beta.data_ptr(),
              mod_s.data_ptr(), mod_t.data_ptr(), mr.data_ptr(), du.data_ptr(), Cc, dg.data_ptr(), dbt.data_ptr(),
              _ptr(dbias), dms.data_ptr(), dmt.data_ptr(), 0, N, H * W, Cc, groups, dtype_code(y.dtype), ws.data_ptr(),
              nbytes, _stream())
    return du, dg, dbt, dbias, dms, dmt


ACT_SILU, ACT_GELU = 0, 1


def act_fwd(x: Tensor, kind: int) -> Tensor:
    """elementwise SiLU / exact GELU of a small f32 tensor (the time-embedding MLPs of UNet2)"""
    require_gpu(x)
    y = torch.empty_like(x)
    _lib.call("cy_act_fwd", x.data_ptr(), y.data_ptr(), x.numel(), kind, _stream())
    return y


def act_bwd(x: Tensor, dy: Tensor, kind: int) -> Tensor:
    dx = torch.empty_like(x)
    _lib.call("cy_act_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), kind, _stream())
    return dx


def sinusoidal_emb(time: Tensor, dim: int) -> Tensor:
    """SinusoidalPosEmb(dim)(time) (contrastyou/arch/unet2.py:161-173): [B] -> [B, dim]"""
    require_gpu(time)
    t = time.detach().float().contiguous()
    out = _f32(t.numel() * dim, t.device).view(t.numel(), dim)
    _lib.call("cy_sinusoidal_emb", t.data_ptr(), out.data_ptr(), t.numel(), dim, _stream())
    return out


def bilinear_fwd(x: Tensor, size: Tuple[int, int]) -> Tensor:
    require_gpu(x)
    x = to_nhwc(x)
    N, Cc, H, W = x.shape
    out = empty_nhwc(N, Cc, size[0], size[1], x.dtype, x.device)
    _lib.call("cy_bilinear_fwd", x.data_ptr(), out.data_ptr(), N, H, W, Cc, size[0], size[1], dtype_code(x.dtype),
              _stream())
    return out


# --------------------------------------------------------------------------- cross-correlation regulariser
def cc_edge_map(image: Tensor, power: float) -> Tensor:
    """image f32 [N, C, H, W], C <= 4 -> [N, 1, H, W]: per-image min/max-normalised edge strength ** power
    (semi_seg/hooks/ccblock.py:287-293,302); two launches"""
    require_gpu(image)
    x = to_nhwc(image.detach().float())
    N, Cc, H, W = x.shape
    out = _f32(N * H * W, x.device).view(N, 1, H, W)
    nbytes = _lib.load().cy_cc_edge_map_ws_bytes(N)
    ws = _ws(nbytes, x.device)
    _lib.call("cy_cc_edge_map", x.data_ptr(), out.data_ptr(), N, H, W, Cc, float(power), ws.data_ptr(), nbytes,
              _stream())
    return out


def entropy_map_fwd(prob: Tensor, slicewise: bool):
    """prob f32 [N, K, H, W] with NHWC memory -> (normalised entropy map [N, 1, H, W], extrema [N, 2]); two launches"""
    require_gpu(prob)
    N, K, H, W = prob.shape
    out = _f32(N * H * W, prob.device).view(N, 1, H, W)
    mm = _f32(N * 2, prob.device).view(N, 2)
    nbytes = _lib.load().cy_entropy_map_ws_bytes(N)
    ws = _ws(nbytes, prob.device)
    _lib.call("cy_entropy_map_fwd", prob.data_ptr(), out.data_ptr(), mm.data_ptr(), N, H * W, K, int(slicewise),
              ws.data_ptr(), nbytes, _stream())
    return out, mm


def entropy_map_bwd(prob: Tensor, mm: Tensor, dmap: Tensor) -> Tensor:
    N, K, H, W = prob.shape
    dp = empty_nhwc(N, K, H, W, torch.float32, prob.device)
    _lib.call("cy_entropy_map_bwd", prob.data_ptr(), mm.data_ptr(), dmap.data_ptr(), dp.data_ptr(), N, H * W, K,
              _stream())
    return dp


def ccloss_fwd(I: Tensor, J: Tensor, win: int, eps: float) -> Tensor:
    """I, J: f32 contiguous [N, 1, H, W] -> scalar CCLoss (contrastyou/losses/cross_correlation.py:22-74); two launches"""
    require_gpu(I, J)
    N, _, H, W = I.shape
    nbytes = _lib.load().cy_ccloss_ws_bytes(N, H, W)
    ws = _ws(nbytes, I.device)
    loss = _f32(1, I.device)
    _lib.call("cy_ccloss_fwd", I.data_ptr(), J.data_ptr(), loss.data_ptr(), N, H, W, win, float(eps), ws.data_ptr(),
              nbytes, _stream())
    return loss.view(())


def ccloss_bwd(I: Tensor, J: Tensor, gscale: Tensor, win: int, eps: float, need_i: bool, need_j: bool):
    N, _, H, W = I.shape
    dI = torch.empty_like(I) if need_i else None
    dJ = torch.empty_like(J) if need_j else None
    _lib.call("cy_ccloss_bwd", I.data_ptr(), J.data_ptr(), gscale.data_ptr(), _ptr(dI), _ptr(dJ), N, H, W, win,
              float(eps), _stream())
    return dI, dJ


# --------------------------------------------------------------------------- adversarial baseline (csrc/cy_disc.hip)
def softmax_cat_fwd(image: Optional[Tensor], logits: Tensor) -> Tensor:
    """image f32 [N, Ci, H, W] with NHWC memory (or None), logits f32 [N, K, H, W] with NHWC memory ->
    rows [N, H, W, Ci + K] = (image, softmax(logits)); one launch"""
    require_gpu(image, logits)
    N, K, H, W = logits.shape
    Ci = 0 if image is None else image.shape[1]
    out = torch.empty((N, H, W, Ci + K), dtype=torch.float32, device=logits.device)
    _lib.call("cy_softmax_cat_fwd", _ptr(image), logits.data_ptr(), out.data_ptr(), N * H * W, Ci, K, _stream())
    return out


def softmax_cat_bwd(logits: Tensor, dout: Tensor, Ci: int) -> Tensor:
    """dout: rows [N, H, W, Ci + K] contiguous -> dlogits [N, K, H, W] with NHWC memory; one launch"""
    N, K, H, W = logits.shape
    d = empty_nhwc(N, K, H, W, torch.float32, logits.device)
    _lib.call("cy_softmax_cat_bwd", logits.data_ptr(), dout.data_ptr(), d.data_ptr(), N * H * W, Ci, K, _stream())
    return d


def _bn_rows_ws(M: int, Cc: int, device):
    nbytes = _lib.load().cy_bn_rows_ws_bytes(M, Cc)
    return _ws(nbytes, device), nbytes


def bn_rows_stats(x2d: Tensor, running_mean: Optional[Tensor] = None, running_var: Optional[Tensor] = None,
                  num_batches_tracked: Optional[Tensor] = None, momentum: float = 0.1) -> Tuple[Tensor, Tensor]:
    """x2d f32 [M, C] contiguous -> (mean [C], biased var [C]); updates the running statistics in place when given
    (nn.BatchNorm2d's rule: unbiased variance, counter + 1); two launches"""
    require_gpu(x2d)
    M, Cc = x2d.shape
    stats = _f32(2 * Cc + 8, x2d.device)
    half = (Cc + 3) // 4 * 4  # keeps `var` 16-byte aligned
    mean, var = stats[:Cc], stats[half:half + Cc]
    ws, nbytes = _bn_rows_ws(M, Cc, x2d.device)
    _lib.call("cy_bn_rows_stats", x2d.data_ptr(), mean.data_ptr(), var.data_ptr(), M, Cc, _ptr(running_mean),
              _ptr(running_var), _ptr(num_batches_tracked), float(momentum), ws.data_ptr(), nbytes, _stream())
    return mean, var


def bn_lrelu_fwd(x2d: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float,
                 slope: float) -> Tensor:
    require_gpu(x2d)
    M, Cc = x2d.shape
    y = torch.empty_like(x2d)
    _lib.call("cy_bn_lrelu_fwd", x2d.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
              y.data_ptr(), M, Cc, float(eps), float(slope), _stream())
    return y


def bn_lrelu_bwd(x2d: Tensor, dy2d: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float,
                 slope: float, batch_stats: bool, need_dx: bool = True, need_sums: bool = True):
    """-> (dx [M, C] or None, dgamma [C], dbeta [C]); reduce (two launches) + apply (one launch).  `need_sums=False`
    (running statistics, no parameter gradient wanted) skips the reduce and returns None for the two sums"""
    M, Cc = x2d.shape
    assert need_sums or not batch_stats, "the batch-statistics data gradient needs dgamma and dbeta"
    dgamma = dbeta = None
    if need_sums:
        half = (Cc + 3) // 4 * 4
        dgb = _f32(2 * Cc + 8, x2d.device)
        dgamma, dbeta = dgb[:Cc], dgb[half:half + Cc]
        ws, nbytes = _bn_rows_ws(M, Cc, x2d.device)
        _lib.call("cy_bn_lrelu_bwd_reduce", x2d.data_ptr(), dy2d.data_ptr(), mean.data_ptr(), var.data_ptr(),
                  gamma.data_ptr(), beta.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), M, Cc, float(eps),
                  float(slope), ws.data_ptr(), nbytes, _stream())
    dx = None
    if need_dx:
        dx = torch.empty_like(x2d)
        _lib.call("cy_bn_lrelu_bwd_apply", x2d.data_ptr(), dy2d.data_ptr(), mean.data_ptr(), var.data_ptr(),
                  gamma.data_ptr(), beta.data_ptr(), _ptr(dgamma), _ptr(dbeta), dx.data_ptr(), M, Cc,
                  float(eps), float(slope), int(batch_stats), _stream())
    return dx, dgamma, dbeta


def leaky_relu_fwd(x: Tensor, slope: float) -> Tensor:
    """x: f32, dense in memory (any dimension order) -> same layout"""
    require_gpu(x)
    y = torch.empty_like(x)
    _lib.call("cy_leaky_relu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), float(slope), _stream())
    return y


def leaky_relu_bwd(x: Tensor, dy: Tensor, slope: float) -> Tensor:
    dx = torch.empty_like(x)
    _lib.call("cy_leaky_relu_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), float(slope), _stream())
    return dx


def sigmoid_bce_fwd(scores: Tensor, label: float) -> Tensor:
    """scores: f32 contiguous, any shape -> scalar BCELoss()(sigmoid(scores), full(label)); two launches"""
    require_gpu(scores)
    n = scores.numel()
    nbytes = _lib.load().cy_sigmoid_bce_ws_bytes(n)
    ws = _ws(nbytes, scores.device)
    loss = _f32(1, scores.device)
    _lib.call("cy_sigmoid_bce_fwd", scores.data_ptr(), float(label), loss.data_ptr(), n, ws.data_ptr(), nbytes,
              _stream())
    return loss.view(())


def sigmoid_bce_bwd(scores: Tensor, label: float, gscale: Tensor) -> Tensor:
    d = torch.empty_like(scores)
    _lib.call("cy_sigmoid_bce_bwd", scores.data_ptr(), float(label), gscale.data_ptr(), d.data_ptr(), scores.numel(),
              _stream())
    return d


# --------------------------------------------------------------------------- the discriminator's 4 x 4 convolutions
def conv4x4_out_hw(H: int, W: int, stride: int, pad: int) -> Tuple[int, int]:
    return (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1


def conv4x4_pack(w: Tensor, transposed: bool) -> Tensor:
    """w: f32 [Cout, Cin, 4, 4] contiguous -> flat [Cout][kh][kw][Cin] (forward) or [Cin][kh][kw][Cout] (transposed:
    what the data gradient reads); one launch"""
    require_gpu(w)
    Cout, Cin = w.shape[0], w.shape[1]
    out = _f32(w.numel(), w.device)
    _lib.call("cy_conv4x4_pack_weights", w.data_ptr(), out.data_ptr(), Cin, Cout, int(transposed), _stream())
    return out


def conv4x4_fwd(xr: Tensor, wp: Tensor, Cout: int, ksize: int, stride: int, pad: int) -> Tensor:
    """xr: f32 [N, H, W, Cin] contiguous, wp from conv4x4_pack(w, False) -> y [N, Ho, Wo, Cout]; one launch"""
    require_gpu(xr, wp)
    N, H, W, Cin = xr.shape
    Ho, Wo = conv4x4_out_hw(H, W, stride, pad)
    y = torch.empty((N, max(Ho, 0), max(Wo, 0), Cout), dtype=torch.float32, device=xr.device)
    _lib.call("cy_conv4x4_fwd", xr.data_ptr(), wp.data_ptr(), y.data_ptr(), N, H, W, Cin, Cout, ksize, stride, pad,
              _stream())
    return y


def conv4x4_dgrad(dyr: Tensor, wpt: Tensor, x_shape, ksize: int, stride: int, pad: int) -> Tensor:
    """dyr: f32 [N, Ho, Wo, Cout] contiguous, wpt from conv4x4_pack(w, True), x_shape = (N, H, W, Cin) -> dx of that
    shape, every element written; one launch"""
    require_gpu(dyr, wpt)
    N, H, W, Cin = x_shape
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dyr.device)
    _lib.call("cy_conv4x4_dgrad", dyr.data_ptr(), wpt.data_ptr(), dx.data_ptr(), N, H, W, Cin, dyr.shape[3], ksize,
              stride, pad, _stream())
    return dx


def conv4x4_wgrad(xr: Tensor, dyr: Tensor, ksize: int, stride: int, pad: int) -> Tensor:
    """xr [N, H, W, Cin], dyr [N, Ho, Wo, Cout], both f32 contiguous -> dw [Cout, Cin, 4, 4]; two launches, the
    partial sums of the output-position ranges are added in a fixed order"""
    require_gpu(xr, dyr)
    N, H, W, Cin = xr.shape
    Cout = dyr.shape[3]
    nbytes = _lib.load().cy_conv4x4_wgrad_ws_bytes(N, H, W, Cin, Cout, ksize, stride, pad)
    ws = _ws(nbytes, xr.device)
    dw = torch.empty((Cout, Cin, 4, 4), dtype=torch.float32, device=xr.device)
    _lib.call("cy_conv4x4_wgrad", xr.data_ptr(), dyr.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, ksize, stride, pad,
              ws.data_ptr(), nbytes, _stream())
    return dw
