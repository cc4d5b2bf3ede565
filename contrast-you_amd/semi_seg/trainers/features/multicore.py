"""`MulticoreTrainer` (semi_seg/trainers/features/multicore.py:10-35): `SemiTrainer` with the multi-prototype epochers;
the criterion's own parameters join the optimizer as a further param group (empty for `MultiCoreKL`)."""
from __future__ import annotations

from typing import Type

from contrastyou.losses.multicore_loss import GeneralOverSegmentedLoss
from contrastyou.trainer.base import _NOT_OPTIMIZER_ARGS

from ..trainer import SemiTrainer
from ...epochers.features import MultiCoreEvalEpocher, MultiCoreTrainEpocher

__all__ = ["MulticoreTrainer"]


class MulticoreTrainer(SemiTrainer):
    _criterion: GeneralOverSegmentedLoss

    def _create_initialized_eval_epoch(self, *, model, loader, **kwargs) -> MultiCoreEvalEpocher:
        epocher = MultiCoreEvalEpocher(model=model, loader=loader, sup_criterion=self._criterion,
                                       cur_epoch=self._cur_epoch, device=self._device, scaler=self.scaler,
                                       accumulate_iter=self._accumulate_iter)
        epocher.init(trainer=self)
        return epocher

    @property
    def train_epocher(self) -> Type[MultiCoreTrainEpocher]:
        return MultiCoreTrainEpocher

    def _init_optimizer(self):
        optimizer = super()._init_optimizer()
        kwargs = {k: v for k, v in self._config["Optim"].items() if k not in _NOT_OPTIMIZER_ARGS}
        optimizer.add_param_group({"params": list(self._criterion.parameters()), **kwargs})
        return optimizer
