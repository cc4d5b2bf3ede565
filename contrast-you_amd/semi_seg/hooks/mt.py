"""Mean-teacher regulariser (semi_seg/hooks/mt.py:49-207): an EMA teacher copy of the model
predicts the unlabeled batch (no grad; train-mode BN, or -- with update_bn, where the EMA also tracks
the running statistics -- every teacher BatchNorm in eval mode, mt.py:162-166), its logits go through
the same affine map, and weight * MSE(softmax(teacher_tf) [hard_clip: its arg-max one-hot, mt.py:190-192],
softmax(student_tf)) is added; after the step the teacher is updated by `EMAUpdater` = cy_ema_update
over every parameter.

Uncertainty-aware mean teacher, "UA-MT" (semi_seg/hooks/mt.py:209-276): the teacher's logits are the mean of one
BN-tracking forward and N forwards of the image plus 0.05 * noise; the MSE against the student counts only where the
entropy of that mean prediction lies below thr = (3/4 + 1/4 * cur_epoch / max_epoch) * ln C, and is divided by
(mask.mean() + 1e-2).  Softmax, entropy, mask, [arg-max one-hot,] MSE and both means are one fused pass each way
(`UAMTLossFn` = cy_uamt_mse_*): no full-size temporary and, unlike the reference's two `.item()`, no host sync.

Interpolation-consistency training, "ICT" (semi_seg/hooks/mt.py:279-319): the teacher predicts the unlabeled batch and
its transformed view in two no-grad forwards (it is in train mode: each has its own batch statistics); under the step's
seed one (lam, index) is drawn for the 2B batch with alpha = 0.2, the student runs on the mixed images
(`ops.mix_images`), and weight * mean((softmax(student) - (lam * p + (1 - lam) * p[index]))^2), p the teacher's
softmax, is added.  `MixSoftmaxMSEFn` (cy_softmax_mixmse_*) recomputes both teacher softmaxes and their blend in
registers: neither probability tensor, nor the gathered copy, nor the mixed target is formed.

All three run on multi-prototype logits up to K = 64 outputs: the plain mean teacher on the row form of
cy_softmax_mse_*, UA-MT and ICT on cy_uamt_mse_row_* and cy_softmax_mixmse_row_* (csrc/cy_wide_reg.hip) past 16."""
from __future__ import annotations

import math
from copy import deepcopy

import torch
from torch import nn

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.meters import AverageValueMeter, MeterInterface
from cyhip import ops
from contrastyou.utils.utils import fix_all_seed_within_context
from cyhip.functions import MixSoftmaxMSEFn, SoftmaxMSEFn, UAMTLossFn, bump_weights_epoch
from semi_seg.hooks.utils import mixup_draw


class EMAUpdater:
    def __init__(self, alpha=0.999, justify_alpha=True, weight_decay=1e-5, update_bn=False) -> None:
        self._alpha, self._weight_decay = alpha, weight_decay
        self._update_bn, self._justify_alpha = update_bn, justify_alpha
        self._global_step = 0

    @torch.no_grad()
    def __call__(self, ema_model: nn.Module, student_model: nn.Module):
        alpha = min(1 - 1 / (self._global_step + 1), self._alpha) if self._justify_alpha else self._alpha
        for e, s in zip(ema_model.parameters(), student_model.parameters()):
            ops.ema_update(e.data, s.data, alpha, self._weight_decay)
        if self._update_bn:
            for (name, eb), (_, sb) in zip(ema_model.named_buffers(), student_model.named_buffers()):
                if "running_mean" in name or "running_var" in name:
                    ops.ema_update(eb.data, sb.data, alpha, self._weight_decay)
        bump_weights_epoch()  # teacher weights changed outside torch's version counter
        self._global_step += 1


def detach_model(model: nn.Module):
    for p in model.parameters():
        p.detach_()
        p.requires_grad_(False)


class MeanTeacherTrainerHook(TrainerHook):

    def __init__(self, *, name: str, model: nn.Module, weight: float, alpha: float = 0.999,
                 weight_decay: float = 1e-5, update_bn=False, num_teachers: int = 1, hard_clip=False):
        super().__init__(hook_name=name)
        if num_teachers > 1:
            raise RuntimeError(f"Current version only support one Teacher, given {num_teachers} Teachers.")
        self._weight = weight
        self._updater = EMAUpdater(alpha=alpha, weight_decay=weight_decay, update_bn=update_bn)
        self._teacher_model = deepcopy(model)
        self._hard_clip = hard_clip
        detach_model(self._teacher_model)

    def __call__(self):
        return _MeanTeacherEpocherHook(name=self._hook_name, weight=self._weight, model=self.trainer._model,
                                       teacher_model=self._teacher_model, updater=self._updater,
                                       hard_clip=self._hard_clip)

    @property
    def teacher_model(self):
        return self._teacher_model

    @property
    def learnable_modules(self):
        return []


class _MeanTeacherEpocherHook(EpocherHook):
    def __init__(self, *, name: str, weight: float, model, teacher_model, updater: EMAUpdater,
                 hard_clip: bool = False) -> None:
        super().__init__(name=name)
        self._weight, self._model, self._teacher_model, self._updater = weight, model, teacher_model, updater
        self._hard_clip = hard_clip
        self._teacher_model.train()
        if updater._update_bn:  # the EMA'd running statistics are the ones to use: freeze every BN to eval()
            for m in self._teacher_model.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters = super().configure_meters_given_epocher(meters)
        meters.register_meter("loss", AverageValueMeter())
        return meters

    def _call_implementation(self, *, unlabeled_image, unlabeled_tf_logits, seed, affine_transformer, **kwargs):
        with torch.no_grad():
            teacher_logits = self._teacher_model(unlabeled_image)
            teacher_logits_tf = affine_transformer(teacher_logits)
            if self._hard_clip:
                # one-hot of the teacher's arg-max class, expressed as logits whose softmax IS that one-hot
                # (exp(-1e4) == 0 in f32), so that the fused softmax-pair MSE kernel applies unchanged
                C = teacher_logits_tf.shape[1]
                hard = torch.nn.functional.one_hot(teacher_logits_tf.argmax(1), C).movedim(-1, 1)
                teacher_logits_tf = hard.to(torch.float32) * 1e4
        loss = SoftmaxMSEFn.apply(teacher_logits_tf.detach(), unlabeled_tf_logits)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss

    def after_batch_update(self, **kwargs):
        self._updater(ema_model=self._teacher_model, student_model=self._model)


def uamt_threshold(num_classes: int, cur_epoch: int, max_epoch: int) -> float:
    """the entropy bound of the UA-MT mask (mt.py:244), in f64 on the host; the kernel takes it rounded to f32"""
    log_c = math.log(num_classes)
    return 3 / 4 * log_c + 1 / 4 * log_c * float(cur_epoch / max_epoch)


class UAMeanTeacherTrainerHook(MeanTeacherTrainerHook):

    def __call__(self):
        return _UAMeanTeacherEpocherHook(name=self._hook_name, weight=self._weight, model=self.trainer._model,
                                         teacher_model=self._teacher_model, updater=self._updater,
                                         hard_clip=self._hard_clip)


class _UAMeanTeacherEpocherHook(_MeanTeacherEpocherHook):

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters = super().configure_meters_given_epocher(meters)
        meters.register_meter("mask", AverageValueMeter())
        return meters

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, **kwargs):
        teacher_logits_tf = self._aggregate_predictions(unlabeled_image=unlabeled_image, N=4,
                                                        affine_transformer=affine_transformer, seed=seed)
        thr = uamt_threshold(unlabeled_tf_logits.shape[1], self.cur_epoch, self.max_epoch)
        loss, mask_mean = UAMTLossFn.apply(teacher_logits_tf, unlabeled_tf_logits, thr, self._hard_clip)
        self.meters["loss"].add(loss.detach())
        self.meters["mask"].add(mask_mean)
        return self._weight * loss

    def _noise(self, like: torch.Tensor, i: int) -> torch.Tensor:
        """the i-th perturbation of the unlabeled batch, before the 0.05 scale (drawn under the step's seed)"""
        return torch.randn_like(like)

    @torch.no_grad()
    def _aggregate_predictions(self, *, unlabeled_image: torch.Tensor, N: int = 8, affine_transformer,
                               seed: int) -> torch.Tensor:
        """mean of the teacher's logits over the clean image (the one forward that writes the BN statistics) and N
        noisy copies, warped once (mt.py:250-268); softmax and entropy of it are taken inside the loss kernel"""
        teacher = self._teacher_model
        with teacher.switch_bn_track(enable=True):
            logits = [teacher(unlabeled_image)]
        with teacher.switch_bn_track(enable=False), fix_all_seed_within_context(seed):
            logits += [teacher(unlabeled_image + self._noise(unlabeled_image, i) * 0.05) for i in range(N)]
        return affine_transformer(torch.stack(logits, dim=0).mean(dim=0))

    @property
    def cur_epoch(self) -> int:
        return self.epocher.cur_epoch

    @property
    def max_epoch(self) -> int:
        return int(self.epocher.trainer._max_epoch)


class ICTMeanTeacherTrainerHook(MeanTeacherTrainerHook):

    def __init__(self, *, name: str, model: nn.Module, weight: float, alpha: float = 0.999, weight_decay: float = 1e-5,
                 update_bn=False):
        super().__init__(name=name, model=model, weight=weight, alpha=alpha, weight_decay=weight_decay,
                         update_bn=update_bn, num_teachers=1, hard_clip=False)

    def __call__(self):
        return _ICTMeanTeacherEpocherHook(name=self._hook_name, weight=self._weight, model=self.trainer._model,
                                          teacher_model=self._teacher_model, updater=self._updater)


class _ICTMeanTeacherEpocherHook(_MeanTeacherEpocherHook):
    MIX_ALPHA = 0.2  # mt.py:312

    def __init__(self, *, name: str, weight: float, model, teacher_model, updater: EMAUpdater) -> None:
        super().__init__(name=name, weight=weight, model=model, teacher_model=teacher_model, updater=updater,
                         hard_clip=False)

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, unlabeled_image_tf, seed, **kwargs):
        with torch.no_grad():
            teacher_logits = torch.cat([self._teacher_model(unlabeled_image),
                                        self._teacher_model(unlabeled_image_tf)], dim=0)
            images = torch.cat([unlabeled_image, unlabeled_image_tf], dim=0)
            n = images.shape[0]
            with fix_all_seed_within_context(seed):
                lam, index = mixup_draw(n, alpha=self.MIX_ALPHA)
            w_self, w_other = ops.mix_weights(lam)
            index = ops.mix_index(index, n, images.device)
            mixed_image = ops.mix_images(images.float(), index, w_self, w_other)
        loss = MixSoftmaxMSEFn.apply(self._model(mixed_image), teacher_logits, index, w_self, w_other)
        if self.meters:
            self.meters["loss"].add(loss.detach())
        return self._weight * loss
