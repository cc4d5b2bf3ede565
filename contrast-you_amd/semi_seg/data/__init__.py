from .device_loader import DeviceLoader, DeviceSliceStore, batch_seed, presize_hw  # noqa: F401
