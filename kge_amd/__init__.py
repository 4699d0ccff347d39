"""kge_amd: HIP kernels for knowledge-graph embedding on gfx950 (the modules are imported on demand)."""

__all__ = ["DeviceSampler", "DeviceKvsAllCollator"]


def __getattr__(name):  # public names, imported on first use (importing the package stays free of torch and the library)
    if name == "DeviceSampler":
        from .sampler import DeviceSampler
        return DeviceSampler
    if name == "DeviceKvsAllCollator":
        from .kvsall import DeviceKvsAllCollator
        return DeviceKvsAllCollator
    raise AttributeError(f"module 'kge_amd' has no attribute {name!r}")
