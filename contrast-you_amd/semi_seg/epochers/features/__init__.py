from .multicore_epocher import MultiCoreEvalEpocher, MultiCoreTrainEpocher  # noqa: F401
