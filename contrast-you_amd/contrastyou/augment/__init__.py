from .device import DevicePipeline, ViewParams, center_crop_offset, rotation_matrix  # noqa: F401
