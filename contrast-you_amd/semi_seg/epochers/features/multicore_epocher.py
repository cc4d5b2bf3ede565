"""`MultiCoreTrainEpocher`, `MultiCoreEvalEpocher` (semi_seg/epochers/features/multicore_epocher.py:13-91): the
semi-supervised step and the evaluation of a network with `multiplier x true_num_classes` outputs under an
over-segmented criterion (`MultiCoreKL` or one of the adaptive criteria with a translation matrix).

Meters and the order of calls are the reference's.  Execution follows semi_seg/epochers/epocher.py here: the supervised
loss goes through `criterion.from_logits` (one fused pass over the K-channel logits), the Dice counts of the reduced
arg-max are taken by `cy_group_dice_counts` (contiguous groups) or `cy_mix_dice_counts` (a criterion that offers `mix()`)
on the device, and the two-stage forward (second stream, HIP-graph replay) is inherited untouched.  Hooks receive the
K-channel logits.  The evaluation's `true_loss` -- the KL term without the criterion's extra terms -- and `loss` come
from `criterion.kl_and_loss_from_logits` where the criterion has one: no softmax or reduced tensor is formed.

`num_classes` is the TRUE class count.  The reference reads it from its global config manager
(`Arch.true_num_classes`); here it is `len(criterion.groups)` (adaptive criteria: their `output_num_classes`), and a
trainer config that carries `Arch.true_num_classes` must agree with it.
"""
from __future__ import annotations

from functools import partial

import torch

from contrastyou.losses.multicore_loss import MultiCoreKL
from contrastyou.meters import AverageValueMeter, MeterInterface
from contrastyou.utils.general import class2one_hot
from semi_seg.epochers.epocher import EvalEpocher, SemiSupervisedEpocher, _scalar, _sup_loss


class _MultiCoreMixin:
    @property
    def num_classes(self) -> int:
        groups = getattr(self._sup_criterion, "groups", None)
        classes = len(groups) if groups is not None else int(self._sup_criterion.output_num_classes)
        config = getattr(self._trainer, "_config", None)  # (no trainer: an epocher run on its own)
        arch = config.get("Arch") if config is not None else None
        if arch is not None and arch.get("true_num_classes") is not None:
            assert int(arch["true_num_classes"]) == classes, (arch["true_num_classes"], classes)
        return classes

    def _contiguous(self, logits) -> bool:
        """the criterion's groups are the contiguous equal partition the fused kernels take"""
        fusable = getattr(self._sup_criterion, "fusable", None)
        return fusable is not None and fusable(logits.shape[1])

    def _add_dice(self, meter, logits, target, group_name):
        mix = getattr(self._sup_criterion, "mix", None)
        if self._contiguous(logits) and mix is not None:
            meter.add_logits(logits, target, group_name=group_name, mix=mix().detach())
        elif self._contiguous(logits):
            meter.add_logits(logits, target, group_name=group_name, groups=self.num_classes)
        else:
            reduced = self._sup_criterion.reduced_simplex(logits.softmax(1))
            meter.add(reduced.max(1)[1], target.squeeze(1), group_name=group_name)


class MultiCoreTrainEpocher(_MultiCoreMixin, SemiSupervisedEpocher):

    def _batch_update(self, *, cur_batch_num: int, labeled_image, labeled_target, labeled_filename, label_group,
                      unlabeled_image, unlabeled_image_tf, seed, unl_group, unl_partition, unlabeled_filename,
                      retain_graph=False, **kwargs):
        warp = partial(self.transform_with_seed, seed=seed, mode="feature")
        self.optimizer_zero(self._optimizer, cur_iter=cur_batch_num)
        with self.autocast:
            label_logits, unlabeled_logits, unlabeled_tf_logits = self.forward_pass(
                labeled_image=labeled_image, unlabeled_image=unlabeled_image, unlabeled_image_tf=unlabeled_image_tf)
            unlabeled_logits_tf = warp(unlabeled_logits)
            sup_loss = _sup_loss(self._sup_criterion, label_logits, labeled_target, self.num_classes)
            reg_loss = self.regularization(
                seed=seed, affine_transformer=warp, labeled_image=labeled_image, labeled_target=labeled_target,
                labeled_filename=labeled_filename, unlabeled_image=unlabeled_image,
                unlabeled_image_tf=unlabeled_image_tf, unlabeled_filename=unlabeled_filename,
                unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_logits_tf=unlabeled_logits_tf,
                label_group=unl_group, partition_group=unl_partition)
        self.scale_loss(sup_loss + reg_loss).backward(retain_graph=retain_graph)
        self.optimizer_step(self._optimizer, cur_iter=cur_batch_num)
        if self.on_master:
            with torch.no_grad():
                self.meters["sup_loss"].add(sup_loss.detach())
                self._add_dice(self.meters["sup_dice"], label_logits, labeled_target, label_group)
                self.meters["reg_loss"].add(_scalar(reg_loss))


class MultiCoreEvalEpocher(_MultiCoreMixin, EvalEpocher):
    def configure_meters(self, meters: MeterInterface) -> MeterInterface:
        meters = super().configure_meters(meters)
        meters.register_meter("true_loss", AverageValueMeter())
        return meters

    def _batch_update(self, *, eval_img, eval_target, eval_group, file_names=None):
        criterion = self._sup_criterion
        with self.autocast:
            logits = self._model(eval_img)
            # `true_loss` = criterion.kl(reduced_simplex, one_hot): for MultiCoreKL that IS the loss (computed once); the
            # adaptive criteria give both from one pass over the logits; any other criterion that adds terms pays the
            # second evaluation
            both = getattr(criterion, "kl_and_loss_from_logits", None)
            if both is not None:
                true_loss, loss = both(logits, eval_target.squeeze(1))
            else:
                loss = true_loss = _sup_loss(criterion, logits, eval_target, self.num_classes)
                if not isinstance(criterion, MultiCoreKL):
                    reduced = criterion.reduced_simplex(logits.softmax(1))
                    true_loss = criterion.kl(reduced, class2one_hot(eval_target.squeeze(1), self.num_classes))
        self.meters["loss"].add(loss.detach())
        self.meters["true_loss"].add(true_loss.detach())
        self._add_dice(self.meters["dice"], logits, eval_target, eval_group)
