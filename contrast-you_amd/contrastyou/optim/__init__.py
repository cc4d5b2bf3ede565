"""Optimizers of the hot path (the reference re-exports torch.optim.*, contrastyou/optim/__init__.py).

Every name a reference yaml's `Optim.name` uses is a flat-buffer optimizer here (flat_optimizer.py): torch.optim's
semantics as ONE HIP kernel launch per parameter group over flat f32 buffers, with the data-parallel gradient
all-reduce (RCCL) folded into `step()`.  `RAdam` is `FusedRAdam` (contrastyou/trainer/base.py:66-75,
config/base.yaml:10-13), `SGD`, `Adam` and `AdamW` are `FusedSGD`, `FusedAdam` and `FusedAdamW`."""
from .flat_optimizer import FlatOptimizer, FlatParams  # noqa: F401
from .flat_teacher import FlatTeacher  # noqa: F401
from .fused_adam import FusedAdam, FusedAdamW  # noqa: F401
from .fused_radam import FusedRAdam  # noqa: F401
from .fused_sgd import FusedSGD  # noqa: F401
from .scheduler import GradualWarmupScheduler  # noqa: F401

RAdam = FusedRAdam
SGD = FusedSGD
Adam = FusedAdam
AdamW = FusedAdamW
