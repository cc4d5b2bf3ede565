"""`MulticoreTrainer` (semi_seg/trainers/features/multicore.py:10-35): `SemiTrainer` with the multi-prototype epochers;
the criterion's own parameters join the optimizer as a further param group (empty for `MultiCoreKL`; the translation
matrix of the adaptive criteria).  Under `FusedRAdam` that group has flat buffers of its own: the matrix's gradient comes
out of `SoftmaxMixKLFn.backward`, passes the softmax of the matrix in autograd and is accumulated in place into the
group's flat gradient buffer, outside the HIP-graph replay of the network passes, which covers the model only.
As in the reference the criterion is a non-trackable buffer of the trainer: the translation matrix is not part of the
trainer's checkpoint."""
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
