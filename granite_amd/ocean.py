"""The ocean's FFT update on an Application's device (gra_ocean_* of include/granite_app.h).

    ocean = Ocean(app, fft_resolution=128, grid_count=4, grid_resolution=32, ocean_size=(128, 128))
    ocean.update(1.5)
    heights = ocean.read("ocean-height-fft-output")              # (128, 128) fp16 bits
    coarse = ocean.read("ocean-gradient-jacobian-output", 3)     # (16, 16, 4)

Keyword arguments are the fields of gra_ocean_config; what is left out keeps the reference's default."""
import ctypes as C

import numpy as np

from . import app as _app
from . import capi

RESOURCES = ["ocean-height-fft-input", "ocean-normal-fft-input", "ocean-displacement-fft-input", "ocean-height-fft-output",
             "ocean-displacement-fft-output", "ocean-normal-fft-output", "ocean-spd-counter", "ocean-gradient-jacobian-output",
             "ocean-height-displacement-output"]
DISTRIBUTIONS = ["height", "displacement", "normal"]
_CHANNELS = {capi.FORMAT_R16_SFLOAT: 1, capi.FORMAT_R16G16_SFLOAT: 2, capi.FORMAT_R16G16B16A16_SFLOAT: 4}


class Ocean:
    def __init__(self, app: "_app.Application", **config):
        self.app, self.lib = app, app.lib
        self.handle = None
        cfg = _app.OceanConfig()
        self.lib.gra_ocean_default_config(C.byref(cfg))
        for key, value in config.items():
            if key not in dict(cfg._fields_):
                raise TypeError(f"Ocean: unknown configuration field {key!r}")
            if key in ("ocean_size", "wind_velocity", "frequency_bands"):
                getattr(cfg, key)[:] = [float(v) for v in value]
            else:
                setattr(cfg, key, value)
        self.config = cfg
        handle = C.c_void_p()
        app._check(self.lib.gra_ocean_create(app.handle, C.byref(cfg), C.byref(handle)))
        self.handle = handle

    def update(self, elapsed_time: float):
        self.app._check(self.lib.gra_ocean_update(self.handle, float(elapsed_time)))

    def describe(self, name: str) -> "_app.OceanResourceInfo":
        info = _app.OceanResourceInfo()
        self.app._check(self.lib.gra_ocean_describe(self.handle, RESOURCES.index(name), C.byref(info)))
        return info

    def read(self, name: str, level: int = 0) -> np.ndarray:
        """A buffer as uint32 (packed half2 per bin), an image level as fp16 bits of shape (h, w) or (h, w, channels)."""
        info = self.describe(name)
        if not info.exists:
            raise capi.GraniteHipError(f"{name} does not exist in this configuration")
        if not info.is_image:
            out = np.empty(info.size_bytes // 4, np.uint32)
        else:
            w, h, c = max(info.width >> level, 1), max(info.height >> level, 1), _CHANNELS[info.format]
            out = np.empty((h, w) if c == 1 else (h, w, c), np.uint16)
        self.app._check(self.lib.gra_ocean_read(self.handle, RESOURCES.index(name), int(level), out.ctypes.data, out.nbytes))
        return out

    def distribution(self, name: str) -> np.ndarray:
        """(N, N, 2) float32: the Phillips distribution the update animates."""
        n = self.config.fft_resolution >> (self.config.displacement_downsample if name == "displacement" else 0)
        out = np.empty((n, n, 2), np.float32)
        self.app._check(self.lib.gra_ocean_distribution(self.handle, DISTRIBUTIONS.index(name), out.ctypes.data))
        return out

    def parameters(self) -> dict:
        out = np.empty(8, np.float32)
        self.app._check(self.lib.gra_ocean_parameters(self.handle, out.ctypes.data))
        return {"heightmap_world_size": out[0:2].copy(), "normalmap_world_size": out[2:4].copy(), "wind_direction": out[4:6].copy(),
                "phillips_L": out[6], "amplitude": out[7]}

    def close(self):
        if self.handle is not None:
            self.lib.gra_ocean_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
