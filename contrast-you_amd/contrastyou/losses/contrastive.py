"""InfoNCE / supervised-contrastive loss with the interface of
contrastyou/losses/contrastive.py:23-100 (`SupConLoss1`), computed by the HIP SupCon kernels:
f32-MFMA similarity GEMM, row statistics with the reference's global-max shift, and the
(G + G^T) P / t backward -- see csrc/cy_contrast.hip.

    criterion(z1, z2, target=list|Tensor|None, mask=None) -> scalar loss
    criterion.sim_exp / .sim_logits / .pos_mask / .neg_mask   (materialised on first access)

`mask` is the reference's: [n, n], 1 = positive, 0 = negative, any other value neither (in no denominator), read as
given -- it need not be symmetric.

The reference asserts unit-norm inputs (AssertionError) and raises RuntimeError on a NaN loss,
both through host syncs.  Here the same conditions are evaluated on the device and checked by
`validate()`; with `defer_checks=False` (default) validate() runs inside forward, exactly like the
reference; the training hooks switch to deferred mode and validate once per epoch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from cyhip import ops
from cyhip.functions import SelfPacedSupConFn, SgemmFn, SupConFn


def is_normalized(feature: Tensor, dim=1) -> bool:
    norms = feature.norm(dim=dim)
    return torch.allclose(norms, torch.ones_like(norms))


_label_cache = {}  # label tuple -> int32 device tensor (a few distinct partitions per dataset)


def _encode_target(target, n: int, device) -> Tensor:
    """labels as int32 codes (equality is all that matters: contrastive.py:41)"""
    if isinstance(target, Tensor):
        t = target.detach().reshape(-1)
        if t.is_floating_point():
            _, t = torch.unique(t, return_inverse=True)
        t = t.to(device=device, dtype=torch.int32)
    else:
        vals = tuple(target)
        assert len(vals) == n, (len(vals), n)
        key = (vals, str(device))
        t = _label_cache.get(key)
        if t is None:
            lut = {}
            host = torch.tensor([lut.setdefault(v, len(lut)) for v in vals], dtype=torch.int32)
            t = ops.pinned.upload(host, device)
            if len(_label_cache) > 512:
                _label_cache.clear()
            _label_cache[key] = t
        return t
    assert t.numel() == n, (t.numel(), n)
    return t.contiguous()


def _rejoin(a: Tensor, b: Tensor) -> Tensor:
    """cat([a, b]) -- without the copy (and, in the backward, without the zero-fill + two slice copies of the
    chunk's gradient) when a and b are the two halves `torch.chunk` made of one contiguous tensor, which is how the
    InfoNCE hook hands the projector's output over (semi_seg/hooks/infonce.py:226-230 in the reference)"""
    base = a._base
    if (base is not None and base is b._base and base.dim() == a.dim() and base.is_contiguous()
            and a.is_contiguous() and b.is_contiguous() and base.shape[0] == a.shape[0] + b.shape[0]
            and base.shape[1:] == a.shape[1:] == b.shape[1:] and a.data_ptr() == base.data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()):
        return base
    return torch.cat([a, b], dim=0)


def _raise_pending(pending, t):
    """the reference's two checks on the device-side evidence (min S_ii, max S_ii, loss) of the calls since the last
    validate(): AssertionError (inputs not unit norm), RuntimeError (NaN loss)"""
    if not pending:
        return
    ends = torch.stack([p[0] for p in pending] + [p[1] for p in pending])  # extreme S_ii = |P_i|^2 / t
    errs = (ends * t - 1).abs().max()
    losses = torch.stack([p[2] for p in pending])
    bad_norm, has_nan = (errs > 1e-4).item(), torch.isnan(losses).any().item()
    assert not bad_norm, "features need to be normalized first"
    if has_nan:
        raise RuntimeError(losses)


class SupConLoss1(nn.Module):
    def __init__(self, temperature=0.07, exclude_other_pos=False):
        super().__init__()
        self._t = temperature
        self._exclude_pos = exclude_other_pos
        self.defer_checks = False
        self._pending = []
        self._last = None

    def forward(self, proj_feat1: Tensor, proj_feat2: Tensor, target=None, mask: Optional[Tensor] = None, **kwargs):
        assert proj_feat1.shape == proj_feat2.shape, (proj_feat1.shape, proj_feat2.shape)
        ops.require_gpu(proj_feat1, proj_feat2)
        n = proj_feat1.size(0)
        dev = proj_feat1.device
        labels = pos = None
        if mask is not None:
            assert mask.shape == torch.Size([n, n])
            # contrastive.py:35-36: pos = mask == 1, neg = mask == 0, any other value is neither; as uint8 codes 1 / 0 / 2
            code = torch.where(mask == 1, 1, torch.where(mask == 0, 0, 2))
            pos = code.to(device=dev, dtype=torch.uint8).contiguous()
        elif target is not None:
            labels = _encode_target(target, n, dev)
        else:
            labels = torch.arange(n, dtype=torch.int32, device=dev)  # SimCLR: only the other view
        P = _rejoin(proj_feat1, proj_feat2)
        loss, diag, stats = SupConFn.apply(P, labels, pos, float(self._t), self._exclude_pos)
        self._last = (P.detach(), stats, labels, pos)
        # device-side evidence for the reference's two checks: one aminmax launch now, the arithmetic in validate()
        mn, mx = torch.aminmax(diag)
        self._pending.append((mn, mx, loss.detach()))
        if not self.defer_checks:
            self.validate()
        return loss

    def validate(self):
        """raise like the reference: AssertionError (inputs not unit norm), RuntimeError (NaN loss)"""
        pending, self._pending = self._pending, []
        _raise_pending(pending, self._t)

    def _matrices(self):
        if self._last is None:
            raise AttributeError("call the criterion first")
        P, stats, labels, pos = self._last  # (the matrices are inspection aids: the similarity is formed on demand)
        S = ops.sgemm(P.float().contiguous(), P.float().contiguous(), 1.0 / float(self._t), b_trans=True)
        return ops.supcon_matrices(S, stats, labels, pos)

    @property
    def sim_logits(self) -> Tensor:
        return self._matrices()[0]

    @property
    def sim_exp(self) -> Tensor:
        return self._matrices()[1]

    @property
    def pos_mask(self) -> Tensor:
        return self._matrices()[2]

    @property
    def neg_mask(self) -> Tensor:
        return self._matrices()[3]


class SelfPacedSupConLoss(nn.Module):
    """`SelfPacedSupConLoss` (contrastyou/losses/contrastive.py:103-212): SupConLoss1 whose positive pairs are
    weighted by a self-paced mask computed (without gradient) from their own log-likelihood,
    hard: [l_ij <= gamma], soft: max(1 - l_ij / gamma, 0); gamma -> infinity recovers SupConLoss1 (the identity
    the reference checks in its __main__, :241-248).

    For embeddings the fused SupCon kernels take (D <= 256, D % 8 == 0) and gamma > 0 the loss runs on
    `SelfPacedSupConFn`: two passes over the similarity tiles forward, one backward, the 2n x 2n matrix never written
    (csrc/cy_contrast.hip).  Otherwise `_composition` runs: the similarity GEMM on the f32 MFMA kernel
    (cyhip.functions.SgemmFn, differentiable) and the 2n x 2n elementwise part as plain autograd, with the reference's
    host syncs.

    The two checks of the reference (unit-norm inputs -> AssertionError, NaN loss -> RuntimeError) follow
    `SupConLoss1`: evaluated on the device, raised by `validate()`; with `defer_checks=False` (default) validate() runs
    inside forward and `downgrade_ratio` is a Python float, in deferred mode `downgrade_ratio` is a 0-dim device
    tensor and forward does not wait for the device -- given a list of labels seen before (cached on the device), a
    label tensor or a mask already on the device; a mask on the host, a new label list or float labels are uploaded or
    encoded with a wait.  `sim_exp`, `sim_logits`, `pos_mask`, `neg_mask` and `sp_mask` are materialised on first
    access; for that the criterion keeps a reference to P, the row statistics and the labels or mask of its last call
    until the next one (at 4096 x 256 that holds 4 MiB of the projector's output alive between steps), as
    `SupConLoss1` does."""

    def __init__(self, temperature=0.07, weight_update="hard", correct_grad=False, **kwargs):
        super().__init__()
        assert weight_update in ("hard", "soft"), weight_update
        self._t, self._weight_update, self._correct_grad = temperature, weight_update, correct_grad
        self._gamma = 1e6
        self.defer_checks = False
        self._pending = []
        self._last = None   # fused path: (P, stats, labels, pos, gamma) of the last call, for the matrices
        self._mats = None   # the five matrices, once formed

    def __repr__(self):
        return f"{self.__class__.__name__} with T: {self._t}, method: {self._weight_update} gamma: {self._gamma}"

    def set_gamma(self, gamma):
        self._gamma = float(gamma)

    @property
    def age_param(self):
        return self._gamma

    def forward(self, proj_feat1: Tensor, proj_feat2: Tensor, target=None, mask: Optional[Tensor] = None, **kwargs):
        assert proj_feat1.shape == proj_feat2.shape, (proj_feat1.shape, proj_feat2.shape)
        ops.require_gpu(proj_feat1, proj_feat2)
        if not (ops.supcon_fused_ok(proj_feat1) and self._gamma > 0):
            return self._composition(proj_feat1, proj_feat2, target, mask)
        n, dev = proj_feat1.shape[0], proj_feat1.device
        labels = pos = None
        if mask is not None:
            assert mask.shape == torch.Size([n, n])
            # contrastive.py:120-121: pos = mask == 1, neg = mask == 0, any other value is neither; uint8 codes 1 / 0 / 2,
            # formed on the device (a mask that lives on the host is copied over first, and that copy makes the host wait)
            mask = mask.to(dev)
            pos = torch.where(mask == 1, 1, torch.where(mask == 0, 0, 2)).to(torch.uint8).contiguous()
        elif target is not None:
            labels = _encode_target(target, n, dev)
        else:
            labels = torch.arange(n, dtype=torch.int32, device=dev)
        P = _rejoin(proj_feat1, proj_feat2)
        loss, ratio, diag, stats = SelfPacedSupConFn.apply(P, labels, pos, float(self._t), self._gamma,
                                                           self._weight_update == "soft", bool(self._correct_grad))
        self._last, self._mats = (P.detach(), stats, labels, pos, self._gamma), None
        mn, mx = torch.aminmax(diag)
        self._pending.append((mn, mx, loss.detach()))
        if self.defer_checks:
            self.downgrade_ratio = ratio
        else:
            self.downgrade_ratio = ratio.item()
            self.validate()
        return loss

    def validate(self):
        """raise like the reference: AssertionError (inputs not unit norm), RuntimeError (NaN loss)"""
        pending, self._pending = self._pending, []
        _raise_pending(pending, self._t)

    def _composition(self, proj_feat1: Tensor, proj_feat2: Tensor, target=None, mask: Optional[Tensor] = None):
        """the loss as a composition of the similarity GEMM and torch elementwise ops on 2n x 2n tensors: what runs
        for widths the fused kernels refuse, and the baseline of tools/bench_selfpaced.py"""
        n, dev = proj_feat1.shape[0], proj_feat1.device
        if mask is not None:
            assert mask.shape == torch.Size([n, n])
            pos = (mask == 1).float().to(dev)
            neg = (mask == 0).float().to(dev)  # (contrastive.py:120-121: other values, e.g. -1, are neither)
        elif target is not None:
            t = _encode_target(target, n, dev)
            pos = torch.eq(t[:, None], t[None, :]).float()
            neg = 1 - pos
        else:
            pos = torch.eye(n, dtype=torch.float, device=dev)
            neg = 1 - pos
        R = 2 * n
        off_diag = 1 - torch.eye(R, dtype=torch.float, device=dev)
        pos_mask, neg_mask = pos.repeat(2, 2) * off_diag, neg.repeat(2, 2) * off_diag
        P = torch.cat([proj_feat1, proj_feat2], dim=0)
        sim = SgemmFn.apply(P, P, 1.0 / self._t)
        norm_err = (sim.diagonal().detach() * self._t - 1).abs().max()
        assert norm_err.item() < 1e-4, "features need to be normalized first"
        sim_logits = sim - sim.max().detach()
        sim_exp = torch.exp(sim_logits)
        pos_count = pos_mask.sum(1)
        denom = ((sim_exp * pos_mask).sum(1, keepdim=True) + (sim_exp * neg_mask).sum(1, keepdim=True))
        llh = sim_logits - torch.log(denom + 1e-16)
        with torch.no_grad():
            l_ij = -llh
            if self._weight_update == "hard":
                w = (l_ij <= self._gamma).float()
            else:
                w = torch.clamp(1 - l_ij / self._gamma, min=0)
            sp_mask = torch.max(w, 1 - pos_mask)
        self._last = None
        self._mats = dict(sim_exp=sim_exp, sim_logits=sim_logits, pos_mask=pos_mask, neg_mask=neg_mask, sp_mask=sp_mask)
        self.downgrade_ratio = torch.masked_select(sp_mask, pos_mask.bool()).mean().item()
        loss = -(((llh * sp_mask) * pos_mask).sum(1) / pos_count).mean()
        if self._correct_grad and self.downgrade_ratio > 0:
            loss = loss / self.downgrade_ratio
        if torch.isnan(loss):
            raise RuntimeError(loss)
        return loss

    def _matrices(self):
        if self._mats is None:
            if self._last is None:
                raise AttributeError("call the criterion first")
            P, stats, labels, pos, gamma = self._last  # (inspection aids: the similarity is formed on demand)
            S = ops.sgemm(P.float().contiguous(), P.float().contiguous(), 1.0 / float(self._t), b_trans=True)
            sim_logits, sim_exp, pos_mask, neg_mask = ops.supcon_matrices(S, stats, labels, pos)
            l_ij = torch.log(stats[:, :1]) - sim_logits
            w = (l_ij <= gamma).float() if self._weight_update == "hard" else torch.clamp(1 - l_ij / gamma, min=0)
            self._mats = dict(sim_exp=sim_exp, sim_logits=sim_logits, pos_mask=pos_mask, neg_mask=neg_mask,
                              sp_mask=torch.max(w, 1 - pos_mask))
        return self._mats

    @property
    def sim_logits(self) -> Tensor:
        return self._matrices()["sim_logits"]

    @property
    def sim_exp(self) -> Tensor:
        return self._matrices()["sim_exp"]

    @property
    def pos_mask(self) -> Tensor:
        return self._matrices()["pos_mask"]

    @property
    def neg_mask(self) -> Tensor:
        return self._matrices()["neg_mask"]

    @property
    def sp_mask(self) -> Tensor:
        return self._matrices()["sp_mask"]
