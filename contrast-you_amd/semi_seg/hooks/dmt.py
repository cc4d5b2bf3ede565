"""Differentiable mean teacher (semi_seg/hooks/dmt.py:48-420): a teacher copy of the model that is not only an EMA of
the student but is itself trained, with first derivatives only, on the labeled batch.

`DifferentiableMeanTeacherTrainerHook(method_name=...)` hands out one of four epocher hooks.  All of them add
weight * MSE(warp(softmax(teacher(unlabeled))), softmax(student(unlabeled_tf))) to the step's loss, the teacher's
PROBABILITIES being warped: a pixel the zero-padded affine map brings in from outside the image carries the all-zero
vector (`SoftmaxGatherMSEFn` = cy_softmax_gathermse_*; the mean-teacher hook warps logits, whose zero padding is the
uniform distribution).  The teacher stays in train mode (its BatchNorm layers use and write batch statistics) except
where "eval" is written below.  T: teacher, S: student, L: meta criterion on the labeled batch.

    "mt"       consistency against T; after the step T <- EMA(T, S).                                   dmt.py:177-197
    "method1"  consistency against T; the state of T is kept.  After the step: T' <- EMA(T, S), g = dL(T')/dT' (train
               mode), T is put back -- the EMA result and the statistics of that pass are discarded -- and T takes one
               Adam step along g.                                                                       dmt.py:258-302
    "method2"  g = dL(T)/dT with T in eval mode; the consistency is taken against T - meta_weight * g (a train-mode pass,
               whose running statistics stay: only the parameters go back, by the reverse arithmetic, not by a copy);
               after the step T <- EMA(T, S).                                                           dmt.py:305-336
    "method4"  before the regularisation: one train-mode pass of T over the unlabeled batch for its statistics, the
               state of T is kept, g = dL(T)/dT in eval mode, T takes one Adam step.  The consistency is taken against
               that T.  After the step T is put back and T <- EMA(T, S).                                 dmt.py:375-420
    "method3"  raises: the reference's DifferentiableMeanTeacherEpocherHook3 calls `mt_update` without its required
               `teacher_model` and `criterion` arguments (dmt.py:356-360), a TypeError on its first step, so there is no
               behaviour to match.

The EMA is EMAUpdater(update_bn=True): parameters and running statistics.  Adam is torch.optim.Adam(lr=meta_weight,
weight_decay=1e-5).  All teacher bookkeeping runs on `FlatTeacher`'s flat buffers: a constant number of launches per step.

The teacher is part of the hook's state dict (`_teacher_model.*`, next to `_model.*`, as in the reference).  The Adam
moments and step count are NOT, as in the reference, whose teacher optimizer is a plain attribute that no checkpoint
sees: a resumed run restarts them from zero.

The reference's construction-time forward and backward of the teacher on one 1x1x224x224 random image (dmt.py:70-73;
methods 1 and 4) is kept: it leaves every parameter with a zero gradient, so that Adam updates all of them from the
first step, and it writes the teacher's running statistics once.  It runs at construction when the model is on the GPU,
otherwise as soon as the trainer has moved the hook there (`after_initialize`, before a checkpoint is resumed; at the
latest when the first epocher hook is handed out): the network has no CPU path.
"""
from __future__ import annotations

from copy import deepcopy
from typing import List, Optional

import torch
from torch import Tensor, nn

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.losses.dice_loss import DiceLoss
from contrastyou.losses.kl import KL_div
from contrastyou.meters import AverageValueMeter, MeterInterface
from contrastyou.optim.flat_teacher import FlatTeacher
from cyhip import ops, parallel
from cyhip.functions import SoftmaxGatherMSEFn, side_pass
from semi_seg.hooks.mt import EMAUpdater

METHODS = ("mt", "method1", "method2", "method4")
ADAM_WEIGHT_DECAY = 1e-5  # dmt.py:66-67


class _switch_model_status:
    """`with _switch_model_status(model, training=False):` -- dmt.py:40-45"""

    def __init__(self, model: nn.Module, *, training: bool):
        self.model, self.training = model, training

    def __enter__(self):
        self.previous = self.model.training
        self.model.train(self.training)

    def __exit__(self, *exc):
        self.model.train(self.previous)
        return False


def teacher_gradient(teacher: FlatTeacher, loss: Tensor) -> None:
    """d loss / d teacher parameters into the teacher's flat gradient buffer.  With a live f32 .grad the kernels add
    weight gradients straight into it and hand autograd nothing, so `torch.autograd.grad` over the parameters would come
    back empty: the buffer is zeroed, the loss is differentiated, and the weight-gradient stream is joined."""
    teacher.zero_grad()
    loss.backward()
    if loss.is_cuda:
        ops.join_side_streams(torch.cuda.current_stream(loss.device))


class DifferentiableMeanTeacherTrainerHook(TrainerHook):

    def __init__(self, *, name: str, model: nn.Module, weight: float, alpha: float = 0.999, weight_decay: float = 1e-5,
                 meta_weight=1e-3, meta_criterion: str, method_name: str):
        if method_name == "method3":
            raise NotImplementedError(
                "method3 cannot run in the reference either: DifferentiableMeanTeacherEpocherHook3 calls mt_update() "
                "without its required `teacher_model` and `criterion` arguments (semi_seg/hooks/dmt.py:356-360)")
        if method_name not in METHODS:
            raise NotImplementedError(method_name)
        if parallel.is_parallel():
            raise NotImplementedError(
                "DifferentiableMeanTeacherTrainerHook is single-process: the teacher's own passes and optimizer are not "
                f"part of the data-parallel step (world size {parallel.world_size()})")
        assert meta_criterion in {"ce", "dice"}, meta_criterion
        super().__init__(hook_name=name)
        self._weight = weight
        self._meta_criterion = KL_div() if meta_criterion == "ce" else DiceLoss(ignore_index=0)
        self._updater = EMAUpdater(alpha=alpha, weight_decay=weight_decay, update_bn=True)
        self._model = model
        self._teacher_model = deepcopy(model)
        self._meta_weight = meta_weight
        self._method_name = method_name
        self.register_non_trackable_buffer("_teacher", FlatTeacher(self._teacher_model))
        self._needs_init = method_name in {"method1", "method4"}
        if next(self._teacher_model.parameters()).is_cuda:
            self._initialize_teacher_gradient()

    def _initialize_teacher_gradient(self) -> None:
        if not self._needs_init:
            return
        self._needs_init = False
        teacher = self._teacher.ensure()
        dev = next(self._teacher_model.parameters()).device
        with side_pass():
            teacher_gradient(teacher, self._teacher_model(torch.randn(1, 1, 224, 224, device=dev)).mean())
        teacher.zero_grad()

    def after_initialize(self):
        """the trainer has moved the hook to its device (and has not resumed a checkpoint yet)"""
        if next(self._teacher_model.parameters()).is_cuda:
            self._teacher.ensure()
            self._initialize_teacher_gradient()

    def __call__(self):
        self._teacher.ensure()
        self._initialize_teacher_gradient()
        cls = {"mt": MTEpocherHook, "method1": DifferentiableMeanTeacherEpocherHook1,
               "method2": DifferentiableMeanTeacherEpocherHook2,
               "method4": DifferentiableMeanTeacherEpocherHook4}[self._method_name]
        return cls(name=self._hook_name, model=self._model, weight=self._weight, meta_criterion=self._meta_criterion,
                   teacher=self._teacher, updater=self._updater, meta_weight=self._meta_weight)

    @property
    def teacher_model(self):
        return self._teacher_model

    @property
    def flat_teacher(self) -> FlatTeacher:
        return self._teacher

    @property
    def learnable_modules(self) -> List[nn.Module]:
        return []

    @property
    def num_classes(self):
        return self._trainer.num_classes


class _BaseDMTEpocherHook(EpocherHook):

    def __init__(self, *, name: str, model: nn.Module, teacher: FlatTeacher, meta_criterion, weight: float,
                 meta_weight: float, updater: EMAUpdater, **kwargs) -> None:
        super().__init__(name=name)
        self._model, self._teacher, self._teacher_model = model, teacher, teacher.model
        self._weight, self._meta_weight = weight, meta_weight
        self._meta_criterion, self._updater = meta_criterion, updater
        self._index_image: Optional[Tensor] = None
        self._teacher_model.train()
        self._model.train()

    model = property(lambda self: self._model)
    teacher_model = property(lambda self: self._teacher_model)

    def _source_map(self, affine_transformer, like: Tensor) -> Tensor:
        """the step's warp as an int32 map: an image of `pixel index + 1` goes through the same nearest-neighbour kernel
        as every other tensor of the step; 0 is what the zero padding leaves"""
        N, _, H, W = like.shape
        idx = self._index_image
        if idx is None or idx.shape != (N, 1, H, W) or idx.device != like.device:
            idx = self._index_image = ops.source_index_image(N, H, W, like.device)
        return ops.source_map_from_warped(affine_transformer(idx))

    def mt_update(self, *, unlabeled_tf_logits, unlabeled_image, affine_transformer) -> Tensor:
        """dmt.py:138-146 against the teacher as it stands (a train-mode pass without gradient)"""
        with torch.no_grad():
            teacher_logits = self._teacher_model(unlabeled_image)
            source_map = self._source_map(affine_transformer, teacher_logits)
        return SoftmaxGatherMSEFn.apply(teacher_logits, source_map, unlabeled_tf_logits)

    def meta_loss(self, labeled_image: Tensor, labeled_target: Tensor, *, training: bool) -> Tensor:
        """the meta criterion of the teacher's prediction of the labeled batch, differentiable in the teacher"""
        with _switch_model_status(self._teacher_model, training=training):
            logits = self._teacher_model(labeled_image)
        return self._meta_criterion.from_logits(logits, labeled_target.squeeze(1))

    def ema(self) -> None:
        self._teacher.ema_from(self._model, self._updater)


class MTEpocherHook(_BaseDMTEpocherHook):

    def configure_meters_given_epocher(self, meters: MeterInterface):
        self.meters.register_meter("loss", AverageValueMeter())

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, **kwargs):
        loss = self.mt_update(unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_image=unlabeled_image,
                              affine_transformer=affine_transformer)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss

    def after_batch_update(self, **kwargs):
        self.ema()


class _TwoMeters(_BaseDMTEpocherHook):

    def configure_meters_given_epocher(self, meters: MeterInterface):
        self.meters.register_meter("consistency_loss", AverageValueMeter())
        self.meters.register_meter("teacher_loss", AverageValueMeter())


class DifferentiableMeanTeacherEpocherHook1(_TwoMeters):
    """update rule 1"""

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, labeled_image,
                             labeled_target, **kwargs):
        loss = self.mt_update(unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_image=unlabeled_image,
                              affine_transformer=affine_transformer)
        self.meters["consistency_loss"].add(loss.detach())
        self._teacher.snapshot()  # with the running statistics this pass wrote
        return self._weight * loss

    def after_batch_update(self, labeled_image: Tensor, labeled_target: Tensor, **kwargs):
        self.ema()  # teacher at t + 1 (the optimizer's zero_grad before it is teacher_gradient's)
        with side_pass():
            meta_loss = self.meta_loss(labeled_image, labeled_target, training=True)
            teacher_gradient(self._teacher, meta_loss)
        self._teacher.restore()  # teacher at t again: the EMA above and this pass's statistics are gone
        self._teacher.adam_step(self._meta_weight, ADAM_WEIGHT_DECAY)
        self.meters["teacher_loss"].add(meta_loss.detach())


class DifferentiableMeanTeacherEpocherHook2(_TwoMeters):
    """update rule 2"""

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, labeled_image,
                             labeled_target, **kwargs):
        with side_pass():
            teacher_loss = self.meta_loss(labeled_image, labeled_target, training=False)
            teacher_gradient(self._teacher, teacher_loss)
        self._teacher.perturb(-self._meta_weight)  # the teacher at t + 1 ...
        loss = self.mt_update(unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_image=unlabeled_image,
                              affine_transformer=affine_transformer)
        self._teacher.perturb(self._meta_weight)  # ... and at t again (its statistics keep this pass)
        self.meters["consistency_loss"].add(loss.detach())
        self.meters["teacher_loss"].add(teacher_loss.detach())
        return self._weight * loss

    def after_batch_update(self, **kwargs):
        self.ema()


class DifferentiableMeanTeacherEpocherHook4(_TwoMeters):
    """update rule 2 with a meta optimizer"""

    def before_regularization(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, labeled_image,
                              labeled_target, **kwargs):
        with torch.no_grad():  # (the reference builds and drops a graph here: only the statistics matter)
            self._teacher_model(unlabeled_image)
        self._teacher.snapshot()
        with side_pass():
            teacher_loss = self.meta_loss(labeled_image, labeled_target, training=False)
            teacher_gradient(self._teacher, teacher_loss)
        self._teacher.adam_step(self._meta_weight, ADAM_WEIGHT_DECAY)  # teacher at t + 1
        self.meters["teacher_loss"].add(teacher_loss.detach())

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, labeled_image,
                             labeled_target, **kwargs):
        loss = self.mt_update(unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_image=unlabeled_image,
                              affine_transformer=affine_transformer)
        self.meters["consistency_loss"].add(loss.detach())
        return self._weight * loss

    def after_batch_update(self, **kwargs):
        self._teacher.restore()
        self.ema()
