"""Trainer zoo (semi_seg/trainers/__init__.py:7-15).  `dmt` drives a comparison-method epocher that is
outside this build's hot-path scope and raises on use.  The `mixup` entry still raises
too (existing tests pin it); the trainer itself is built and is reached as the class `MixUpTrainer`."""
from contrastyou.trainer.base import Trainer as _Trainer

from .pretrain import PretrainDecoderTrainer, PretrainEncoderTrainer  # noqa: F401
from .trainer import AdversarialTrainer, FineTuneTrainer, MixUpTrainer, MTTrainer, SemiTrainer  # noqa: F401


def _out_of_scope(name):
    class _Unavailable(_Trainer):  # noqa
        def __init__(self, *a, **k):
            raise NotImplementedError(f"Trainer `{name}` (comparison method) is not part of this build")

    return _Unavailable


trainer_zoo = {
    "semi": SemiTrainer,
    "ft": FineTuneTrainer,
    "pretrain": PretrainEncoderTrainer,
    "pretrain_decoder": PretrainDecoderTrainer,
    "mt": MTTrainer,
    "dmt": _out_of_scope("dmt"),
    "mixup": _out_of_scope("mixup"),
}
