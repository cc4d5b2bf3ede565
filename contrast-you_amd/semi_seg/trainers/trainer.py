"""`SemiTrainer`, `FineTuneTrainer`, `MTTrainer`, `MixUpTrainer`, `AdversarialTrainer` (semi_seg/trainers/trainer.py:
27-167, 199-260): which epocher runs a training epoch and how evaluation is wired (teacher model for mean teacher).
"""
from __future__ import annotations

import json
import os
from pathlib import Path
from typing import Any, Dict, Type

import torch
from torch import nn

from contrastyou import optim
from contrastyou.arch.discriminator import Discriminator
from contrastyou.trainer.base import _NOT_OPTIMIZER_ARGS, Trainer
from contrastyou.utils.utils import fix_all_seed_within_context
from semi_seg.epochers.comparable import AdversarialEpocher, MixupEpocher
from semi_seg.epochers.epocher import (EpocherBase, EvalEpocher, FineTuneEpocher, InferenceEpocher,
                                       SemiSupervisedEpocher)
from semi_seg.hooks import MeanTeacherTrainerHook


class SemiTrainer(Trainer):
    activate_hooks = True

    def __init__(self, *, model: nn.Module, labeled_loader, unlabeled_loader, val_loader, test_loader, criterion,
                 save_dir: str, max_epoch: int = 100, num_batches: int = 100, device="cpu", disable_bn: bool,
                 two_stage: bool, config: Dict[str, Any], enable_scale=True, accumulate_iter: int = 1,
                 **kwargs) -> None:
        super().__init__(model=model, criterion=criterion, tra_loader=None, val_loader=val_loader, save_dir=save_dir,
                         max_epoch=max_epoch, num_batches=num_batches, device=device, config=config,
                         enable_scale=enable_scale, accumulate_iter=accumulate_iter, **kwargs)
        del self._tra_loader
        self._labeled_loader = labeled_loader
        self._unlabeled_loader = unlabeled_loader
        self._val_loader = val_loader
        self._test_loader = test_loader
        self._disable_bn = disable_bn
        self._two_stage = two_stage

    @property
    def train_epocher(self) -> Type[EpocherBase]:
        return SemiSupervisedEpocher

    def _create_initialized_tra_epoch(self, **kwargs) -> EpocherBase:
        epocher = self.train_epocher(
            model=self._model, optimizer=self._optimizer, labeled_loader=self._labeled_loader,
            unlabeled_loader=self._unlabeled_loader, sup_criterion=self._criterion, num_batches=self._num_batches,
            cur_epoch=self._cur_epoch, device=self._device, two_stage=self._two_stage, disable_bn=self._disable_bn,
            scaler=self.scaler, accumulate_iter=self._accumulate_iter)
        epocher.init(trainer=self)
        return epocher

    def _create_initialized_eval_epoch(self, *, model, loader, **kwargs) -> EpocherBase:
        epocher = EvalEpocher(model=model, loader=loader, sup_criterion=self._criterion, cur_epoch=self._cur_epoch,
                              device=self._device, scaler=self.scaler, accumulate_iter=self._accumulate_iter)
        epocher.init(trainer=self)
        return epocher

    def inference(self, checkpoint_path: str = None, checkpoint_name: str = "best.pth", save_dir: str = None,
                  enable_prediction_save=False, **kwargs):
        """load `checkpoint_name`, evaluate the test loader, write inference_result.json
        (trainer.py:71-113; per-scan re-batching of the loader is the data layer's job)"""
        checkpoint_path = checkpoint_path or self.absolute_save_dir
        if not os.path.isabs(checkpoint_path):
            raise ValueError(f"`checkpoint_path` must be an absolute path, given {checkpoint_path}")
        self.resume_from_path(str(checkpoint_path), name=checkpoint_name)
        save_dir = save_dir or self.absolute_save_dir
        # (trainer.py:107-123 `_inference`: an InferenceEpocher over the test loader)
        epocher = InferenceEpocher(model=self._model, loader=self._test_loader, sup_criterion=self._criterion,
                                   cur_epoch=self._cur_epoch, device=self._device, scaler=self.scaler,
                                   accumulate_iter=self._accumulate_iter,
                                   enable_prediction_saver=enable_prediction_save, save_dir=save_dir)
        epocher.init(trainer=self)
        epocher.run()
        metrics, score = epocher.get_metric(), epocher.get_score()
        Path(save_dir).mkdir(exist_ok=True, parents=True)
        with open(os.path.join(save_dir, "inference_result.json"), "w") as f:
            json.dump(metrics, f, indent=4)
        return metrics, score


class FineTuneTrainer(SemiTrainer):
    activate_hooks = False

    @property
    def train_epocher(self) -> Type[EpocherBase]:
        return FineTuneEpocher


class MTTrainer(SemiTrainer):
    """validation/test run on the TEACHER of the (single) mean-teacher hook (trainer.py:125-167)"""

    def eval_epoch(self, *, model, loader, **kwargs):
        mt_hook = [h for h in self._hooks if isinstance(h, MeanTeacherTrainerHook)]
        assert len(mt_hook) == 1, mt_hook
        return super().eval_epoch(model=mt_hook[0].teacher_model, loader=loader, **kwargs)


class MixUpTrainer(SemiTrainer):
    """MixUp baseline (trainer.py:207-212): `MixupEpocher` with hooks, `MixUpTrainHook` the one it is meant for.

    Single process only: the hook runs a second forward of the model inside the regularisation, which the
    data-parallel step does not wrap."""
    activate_hooks = True

    def __init__(self, *, model: nn.Module, labeled_loader, unlabeled_loader, val_loader, test_loader, criterion,
                 save_dir: str, max_epoch: int = 100, num_batches: int = 100, device="cpu", disable_bn: bool,
                 two_stage: bool, config: Dict[str, Any], enable_scale=True, accumulate_iter: int = 1,
                 **kwargs) -> None:
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "MixUpTrainer is single-process: the mixed pass of its hook is not part of the data-parallel step "
                f"(world size {dist.get_world_size()})")
        super().__init__(model=model, labeled_loader=labeled_loader, unlabeled_loader=unlabeled_loader,
                         val_loader=val_loader, test_loader=test_loader, criterion=criterion, save_dir=save_dir,
                         max_epoch=max_epoch, num_batches=num_batches, device=device, disable_bn=disable_bn,
                         two_stage=two_stage, config=config, enable_scale=enable_scale,
                         accumulate_iter=accumulate_iter, **kwargs)

    @property
    def train_epocher(self) -> Type[EpocherBase]:
        return MixupEpocher


class AdversarialTrainer(SemiTrainer):
    """adversarial training without hooks (trainer.py:215-260): a `Discriminator(input_dim, hidden_dim=64)` built under
    the config's RandomSeed on [image,] softmax(logits), with an optimizer of its own from `config["Optim"]`.  The
    discriminator (parameters and BatchNorm buffers, `module_state["_discriminator.*"]`) and its optimizer
    (`other_state["_dis_optimizer"]`) are part of the checkpoint.

    Single process only: two flat-buffer optimizers would both write the process-wide early-bucket switch
    (`cyhip.ops.DP_EARLY`) from their own gradient volume in a data-parallel run."""
    activate_hooks = False

    def __init__(self, *, model: nn.Module, labeled_loader, unlabeled_loader, val_loader, test_loader, criterion,
                 save_dir: str, max_epoch: int = 100, num_batches: int = 100, device="cpu", disable_bn: bool,
                 two_stage: bool, config: Dict[str, Any], reg_weight: int, dis_consider_image: bool = False,
                 **kwargs) -> None:
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "AdversarialTrainer is single-process: its two FusedRAdam optimizers would both set cyhip.ops.DP_EARLY "
                f"from their own gradient size (world size {dist.get_world_size()})")
        super().__init__(model=model, labeled_loader=labeled_loader, unlabeled_loader=unlabeled_loader,
                         val_loader=val_loader, test_loader=test_loader, criterion=criterion, save_dir=save_dir,
                         max_epoch=max_epoch, num_batches=num_batches, device=device, disable_bn=disable_bn,
                         two_stage=two_stage, config=config, **kwargs)
        input_dim = self._model._input_dim + self._model.num_classes if dis_consider_image else self._model.num_classes
        self._dis_consider_image = dis_consider_image
        with fix_all_seed_within_context(self._config.get("RandomSeed", 10)):
            self._discriminator = Discriminator(input_dim=input_dim, hidden_dim=64)
        self._discriminator.to(self._device)
        spec = self._config["Optim"]
        self._dis_optimizer = getattr(optim, spec["name"])(
            params=[p for p in self._discriminator.parameters() if p.requires_grad],
            **{k: v for k, v in spec.items() if k not in _NOT_OPTIMIZER_ARGS})
        self._reg_weight = float(reg_weight)

    @property
    def train_epocher(self) -> Type[EpocherBase]:
        return AdversarialEpocher

    def _create_initialized_tra_epoch(self, **kwargs) -> EpocherBase:
        epocher = self.train_epocher(
            model=self._model, optimizer=self._optimizer, labeled_loader=self._labeled_loader,
            unlabeled_loader=self._unlabeled_loader, sup_criterion=self._criterion, num_batches=self._num_batches,
            cur_epoch=self._cur_epoch, device=self._device, two_stage=self._two_stage, disable_bn=self._disable_bn,
            discriminator=self._discriminator, disc_optimizer=self._dis_optimizer, reg_weight=self._reg_weight,
            dis_consider_image=self._dis_consider_image, scaler=self.scaler)
        epocher.init(trainer=self)
        return epocher
