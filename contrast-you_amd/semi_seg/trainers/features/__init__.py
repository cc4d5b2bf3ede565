from .multicore import MulticoreTrainer  # noqa: F401
