"""`AdversarialEpocher` (semi_seg/epochers/comparable.py:93-200 of the reference): the adversarial-training baseline;
`MixupEpocher` (comparable.py:14-90): the MixUp baseline, documented at the class.

One step, in the reference's order:
  G  zero the segmentation optimizer; forward the labeled batch, supervised loss; with reg_weight > 0 forward the
     unlabeled batch and generator_err = BCE(D(unlabeled), 1); backward sup_loss + reg_weight * generator_err; step;
  D  zero the discriminator's gradients; disc_loss = BCE(D(labeled, detached), 1) + BCE(D(unlabeled, detached), 0);
     backward disc_loss * reg_weight; step the discriminator's optimizer.
`D(...)` is `Discriminator.scores_from_logits` (softmax + concat fused, NHWC f32 throughout) and BCE the fused
sigmoid + BCE kernel (cyhip.functions.SigmoidBCEFn); no autocast is entered here, as in the reference.

What differs from the reference is confined to execution:
  * the G step runs the discriminator on detached parameters: the reference accumulates discriminator parameter
    gradients there and throws them away (`discriminator.zero_grad()` opens its D step), so the weight-gradient GEMMs
    and BatchNorm parameter gradients of that pass are skipped; the gradient on the logits and both optimizers'
    results are the same;
  * the discriminator's gradients are zeroed through its optimizer (a flat-buffer optimizer keeps its gradient views
    attached that way);
  * meters take device scalars (no `.item()` per batch), statistics are sampled as in the other epochers.
The two U-Net passes run eagerly on the current stream: no graph replay, no second stream.
"""
from __future__ import annotations

import random
from functools import partial

import torch
from torch import nn

from contrastyou.meters import AverageValueMeter, MeterInterface
from contrastyou.utils.utils import get_lrs_from_optimizer
from cyhip.functions import SigmoidBCEFn
from semi_seg.epochers.epocher import SemiSupervisedEpocher, _scalar, _sup_loss

__all__ = ["AdversarialEpocher", "MixupEpocher"]

TRUE_LABEL, FAKE_LABEL = 1.0, 0.0


class AdversarialEpocher(SemiSupervisedEpocher):

    def __init__(self, *, model: nn.Module, optimizer, labeled_loader, unlabeled_loader, sup_criterion,
                 num_batches: int, cur_epoch=0, device="cpu", two_stage: bool = False, disable_bn: bool = False,
                 discriminator=None, disc_optimizer=None, reg_weight=None, dis_consider_image: bool,
                 **kwargs) -> None:
        super().__init__(model=model, optimizer=optimizer, labeled_loader=labeled_loader,
                         unlabeled_loader=unlabeled_loader, sup_criterion=sup_criterion, num_batches=num_batches,
                         cur_epoch=cur_epoch, device=device, two_stage=two_stage, disable_bn=disable_bn, **kwargs)
        assert isinstance(discriminator, nn.Module)
        assert isinstance(disc_optimizer, torch.optim.Optimizer)
        self._discriminator = discriminator
        self._discr_optimizer = disc_optimizer
        self._reg_weight = float(reg_weight)
        self._dis_consider_image = dis_consider_image
        self._unlabeled_iter = None

    def _run(self, **kwargs):
        self.meters["lr"].add(get_lrs_from_optimizer(self._optimizer))
        self._model.train()
        return self._run_implementation(**kwargs)

    def configure_meters(self, meters: MeterInterface) -> MeterInterface:
        meters = super().configure_meters(meters)
        meters.delete_meter("reg_loss")
        with meters.focus_on("adv_reg"):
            meters.register_meter("dis_loss", AverageValueMeter())
            meters.register_meter("gen_loss", AverageValueMeter())
            meters.register_meter("reg_weight", AverageValueMeter())
        return meters

    @property
    def unlabeled_iter(self):
        """one iterator per epocher, created at the first unlabeled batch (never with reg_weight == 0)"""
        if self._unlabeled_iter is None:
            self._unlabeled_iter = iter(self._unlabeled_loader)
        return self._unlabeled_iter

    def _discriminate(self, image, logits, param_grads: bool):
        return self._discriminator.scores_from_logits(image if self._dis_consider_image else None, logits,
                                                      param_grads=param_grads)

    def _run_implementation(self, **kwargs):
        with self.meters.focus_on("adv_reg"):
            self.meters["reg_weight"].add(self._reg_weight)
        adversarial = self._reg_weight > 0
        for self.cur_batch_num, labeled_data in zip(self.indicator, self._labeled_loader):
            (labeled_image, _), labeled_target, _, _, label_group = self._unzip_data(labeled_data, self._device)
            unlabeled_image = None
            if adversarial:
                (unlabeled_image, _), _, _, _, _ = self._unzip_data(next(self.unlabeled_iter), self._device)
            self._adversarial_step(labeled_image, labeled_target, label_group, unlabeled_image)
            self._report(self.cur_batch_num, self.cur_batch_num == self.num_batches - 1)

    def _adversarial_step(self, labeled_image, labeled_target, label_group, unlabeled_image):
        adversarial = unlabeled_image is not None
        zero = torch.zeros((), device=self.device, dtype=torch.float)
        # ---- segmentation network
        self._optimizer.zero_grad()
        labeled_logits = self._model(labeled_image)
        sup_loss = _sup_loss(self._sup_criterion, labeled_logits, labeled_target, self.num_classes)
        generator_err, unlabeled_logits = zero, None
        if adversarial:
            unlabeled_logits = self._model(unlabeled_image)
            generator_err = SigmoidBCEFn.apply(self._discriminate(unlabeled_image, unlabeled_logits, False),
                                               TRUE_LABEL)
            generator_loss = sup_loss + self._reg_weight * generator_err
        else:
            generator_loss = sup_loss
        generator_loss.backward()
        self._optimizer.step()
        if self.on_master:
            with torch.no_grad():
                self.meters["sup_loss"].add(sup_loss.detach())
                self.meters["sup_dice"].add_logits(labeled_logits, labeled_target, group_name=label_group)
                with self.meters.focus_on("adv_reg"):
                    self.meters["gen_loss"].add(generator_err.detach())
        # ---- discriminator: maximise log D(labeled) + log(1 - D(unlabeled))
        disc_loss = zero
        if adversarial:
            self._discr_optimizer.zero_grad()
            err_labeled = SigmoidBCEFn.apply(self._discriminate(labeled_image, labeled_logits.detach(), True),
                                             TRUE_LABEL)
            err_unlabeled = SigmoidBCEFn.apply(self._discriminate(unlabeled_image, unlabeled_logits.detach(), True),
                                               FAKE_LABEL)
            disc_loss = err_labeled + err_unlabeled
            (disc_loss * self._reg_weight).backward()
            self._discr_optimizer.step()
        if self.on_master:
            with self.meters.focus_on("adv_reg"):
                self.meters["dis_loss"].add(disc_loss.detach())


class MixupEpocher(SemiSupervisedEpocher):
    """`MixupEpocher` (semi_seg/epochers/comparable.py:14-90 of the reference): no unlabeled image takes part.  One
    forward over cat([labeled_image, labeled_image_tf]), the supervised loss on the first half, and the hooks'
    regularisers on the labeled batch, its transformed view and the transformed target (`MixUpTrainHook`).  The
    unlabeled loader is still drawn from, as in the reference, so that the data order of a run matches the baselines'.
    The pass runs eagerly on the current stream: no graph replay, no second stream.  Meters take device scalars."""

    def _forward_pass(self, *, labeled_image, labeled_image_tf, **kwargs):
        predict_logits = self._model(torch.cat([labeled_image, labeled_image_tf], dim=0))
        label_logits, labeled_tf_logits = torch.chunk(predict_logits, 2, dim=0)
        return label_logits, labeled_tf_logits

    def _run_implement(self):
        if len(self._unlabeled_loader) == 0:  # fully supervised: the labeled stream doubles as unlabeled
            self._unlabeled_loader = self._labeled_loader
        batches = zip(self.indicator, self._labeled_loader, self._unlabeled_loader)
        for self.cur_batch_num, labeled_data, unlabeled_data in batches:
            seed = random.randint(0, int(1e7))
            (labeled_image, _), labeled_target, labeled_filename, _, label_group = \
                self._unzip_data(labeled_data, self._device)
            (unlabeled_image, _), _, unlabeled_filename, unl_partition, unl_group = \
                self._unzip_data(unlabeled_data, self._device)
            labeled_image_tf = self.transform_with_seed(labeled_image, seed=seed, mode="image")
            labeled_target_tf = self.transform_with_seed(labeled_target.float(), seed=seed, mode="feature")
            self.batch_update(
                cur_batch_num=self.cur_batch_num, labeled_image=labeled_image, labeled_image_tf=labeled_image_tf,
                labeled_target=labeled_target, labeled_target_tf=labeled_target_tf, labeled_filename=labeled_filename,
                label_group=label_group, unlabeled_image=unlabeled_image, seed=seed, unl_group=unl_group,
                unl_partition=unl_partition, unlabeled_filename=unlabeled_filename, retain_graph=self.retain_graph)
            self._report(self.cur_batch_num, self.cur_batch_num == self.num_batches - 1)

    def _batch_update(self, *, cur_batch_num: int, labeled_image, labeled_target, labeled_image_tf, labeled_target_tf,
                      labeled_filename, label_group, seed, unl_group, unl_partition, unlabeled_filename,
                      retain_graph=False, **kwargs):
        self.optimizer_zero(self._optimizer, cur_iter=cur_batch_num)
        with self.autocast:
            label_logits, labeled_tf_logits = self.forward_pass(labeled_image=labeled_image,
                                                                labeled_image_tf=labeled_image_tf)
            sup_loss = _sup_loss(self._sup_criterion, label_logits, labeled_target, self.num_classes)
            reg_loss = self.regularization(
                seed=seed, labeled_image=labeled_image, labeled_target=labeled_target,
                labeled_image_tf=labeled_image_tf, labeled_target_tf=labeled_target_tf,
                labeled_filename=labeled_filename,
                affine_transformer=partial(self.transform_with_seed, seed=seed, mode="feature"))
        self.scale_loss(sup_loss + reg_loss).backward(retain_graph=retain_graph)
        self.optimizer_step(self._optimizer, cur_iter=cur_batch_num)
        if self.on_master:
            with torch.no_grad():
                self.meters["sup_loss"].add(sup_loss.detach())
                self.meters["sup_dice"].add_logits(label_logits, labeled_target, group_name=label_group)
                self.meters["reg_loss"].add(_scalar(reg_loss))
