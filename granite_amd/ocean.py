"""The ocean's FFT and LOD updates on an Application's device (gra_ocean_* of include/granite_app.h).

    ocean = Ocean(app, fft_resolution=128, grid_count=4, grid_resolution=32, ocean_size=(128, 128))
    ocean.update(1.5)
    heights = ocean.read("ocean-height-fft-output")              # (128, 128) fp16 bits
    coarse = ocean.read("ocean-gradient-jacobian-output", 3)     # (16, 16, 4)

    ocean = Ocean(app, lod_update=1, grid_count=16, grid_resolution=32, fft_resolution=128, ocean_size=(256, 256))
    ocean.set_camera((3.0, 5.0, -2.0), planes)                   # planes: six (x, y, z, w), inside where dot >= 0
    ocean.update(0.0)                                            # both passes
    draws = ocean.read("ocean-lod-counter").reshape(8, 8)        # eight indirect draws
    vertices, indices = ocean.mesh(0)                            # the finest LOD mesh; ocean.mesh("border")

Keyword arguments are the fields of gra_ocean_config; what is left out keeps the reference's default."""
import ctypes as C

import numpy as np

from . import app as _app
from . import capi

RESOURCES = ["ocean-height-fft-input", "ocean-normal-fft-input", "ocean-displacement-fft-input", "ocean-height-fft-output",
             "ocean-displacement-fft-output", "ocean-normal-fft-output", "ocean-spd-counter", "ocean-gradient-jacobian-output",
             "ocean-height-displacement-output"]
# ids 9 .. 11: they exist only in an ocean created with lod_update
LOD_RESOURCES = ["ocean-lods", "ocean-lod-counter", "ocean-lod-data"]
ALL_RESOURCES = RESOURCES + LOD_RESOURCES
MESH_BORDER = 0xffffffff
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
            if key in ("ocean_size", "wind_velocity", "frequency_bands", "center_position"):
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
        self.app._check(self.lib.gra_ocean_describe(self.handle, ALL_RESOURCES.index(name), C.byref(info)))
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
        self.app._check(self.lib.gra_ocean_read(self.handle, ALL_RESOURCES.index(name), int(level), out.ctypes.data, out.nbytes))
        return out

    def set_camera(self, position, planes):
        """The camera of the next update's LOD pass: position (3 floats) and six planes (6 x 4 floats)."""
        pos = (C.c_float * 3)(*[float(v) for v in position])
        pl = (C.c_float * 24)(*[float(v) for v in np.asarray(planes, np.float32).reshape(24)])
        self.app._check(self.lib.gra_ocean_set_camera(self.handle, pos, pl))

    def draw_info(self) -> "_app.OceanDrawInfo":
        info = _app.OceanDrawInfo()
        self.app._check(self.lib.gra_ocean_draw_info(self.handle, C.byref(info)))
        return info

    def mesh_info(self, which) -> "_app.OceanMeshInfo":
        info = _app.OceanMeshInfo()
        self.app._check(self.lib.gra_ocean_mesh_describe(self.handle, MESH_BORDER if which == "border" else int(which), C.byref(info)))
        return info

    def mesh(self, which):
        """which = 0 .. lods - 1 -> (vertices (k, 8) uint8: pos[4], weights[4]; indices uint16); "border" -> (positions (k, 3) float32, indices)"""
        info = self.mesh_info(which)
        if not info.exists:
            raise capi.GraniteHipError(f"mesh {which!r} does not exist in this configuration")
        vertices = np.empty((info.vertex_count, 3), np.float32) if which == "border" else np.empty((info.vertex_count, 8), np.uint8)
        indices = np.empty(info.index_count, np.uint16)
        assert vertices.nbytes == info.vertex_count * info.vertex_stride and info.index_stride == 2
        self.app._check(self.lib.gra_ocean_mesh_read(self.handle, MESH_BORDER if which == "border" else int(which), vertices.ctypes.data, indices.ctypes.data))
        return vertices, indices

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
