"""`AdversarialEpocher` (semi_seg/epochers/comparable.py:93-200 of the reference): the adversarial-training baseline.

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

import torch
from torch import nn

from contrastyou.meters import AverageValueMeter, MeterInterface
from contrastyou.utils.utils import get_lrs_from_optimizer
from cyhip.functions import SigmoidBCEFn
from semi_seg.epochers.epocher import SemiSupervisedEpocher, _sup_loss

__all__ = ["AdversarialEpocher"]

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
