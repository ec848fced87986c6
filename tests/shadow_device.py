"""Device-side copies of a tests/shadow_cases.py case and the shadow launches on them (tests/test_gpu_shadows.py)."""
import numpy as np

from granite_amd import capi

MAP_FORMATS = {2: capi.FORMAT_R32G32_SFLOAT, 0: capi.FORMAT_D16_UNORM, 1: capi.FORMAT_D32_SFLOAT}


def tight(gr):
    return lambda w, h, fmt, role, name: capi.DeviceImage(gr, w, h, fmt)


def map_format(maps, mode):
    import shadow_cases as sc
    return MAP_FORMATS[sc.map_format_code(maps, mode)]


def directional_args(case, make_image, in_place=True):
    """-> (gr_directional_light_args, {name: image}); make_image(width, height, format, role, name) as tests/gpu_scene.py's"""
    w, h = case["width"], case["height"]
    imgs = {
        "albedo": make_image(w, h, capi.FORMAT_R8G8B8A8_SRGB, "in", "albedo").upload(case["albedo"]),
        "normal": make_image(w, h, capi.FORMAT_A2B10G10R10_UNORM_PACK32, "in", "normal").upload(case["normal"]),
        "pbr": make_image(w, h, capi.FORMAT_R8G8_UNORM, "in", "pbr").upload(case["pbr"]),
        "depth": make_image(w, h, capi.FORMAT_D32_SFLOAT, "in", "depth").upload(case["depth"]),
        "hdr": make_image(w, h, capi.FORMAT_R16G16B16A16_SFLOAT, "rmw" if in_place else "out", "hdr"),
    }
    a = capi.DirectionalLightArgs()
    a.albedo, a.normal, a.pbr, a.depth, a.hdr = (imgs[k].desc for k in ("albedo", "normal", "pbr", "depth", "hdr"))
    if in_place:
        imgs["hdr"].upload(case["emissive"])
        a.emissive = imgs["hdr"].desc
    else:
        imgs["emissive"] = make_image(w, h, capi.FORMAT_R16G16B16A16_SFLOAT, "in", "emissive").upload(case["emissive"])
        imgs["hdr"].upload(np.full_like(case["emissive"], 0x7e00))  # NaN-fill: every pixel must be written
        a.emissive = imgs["emissive"].desc
    a.inv_view_projection[:] = [float(v) for v in case["inv_view_projection"]]
    a.directional.inv_view_proj_col2[:] = [float(v) for v in case["inv_view_projection"][8:12]]
    for key in ("color", "camera_pos", "direction", "camera_front"):
        getattr(a.directional, key)[:] = [float(v) for v in case[key]]
    a.directional.cascade_log_bias = float(case["cascade_log_bias"])
    a.directional.inv_resolution[:] = (1.0 / w, 1.0 / h)
    a.flags = capi.LIGHTING_AMBIENT_FALLBACK_BIT if case["fallback"] else 0
    if case.get("ambient_occlusion") is not None:
        ao = case["ambient_occlusion"]
        imgs["ambient_occlusion"] = make_image(ao.shape[1], ao.shape[0], capi.FORMAT_R8_UNORM, "in", "ambient_occlusion").upload(ao)
        a.ambient_occlusion = imgs["ambient_occlusion"].desc
        a.flags |= capi.LIGHTING_AMBIENT_OCCLUSION_BIT
    a.mode = case["mode"]
    maps = case["maps"]
    a.layers = maps.shape[0]
    fmt = map_format(maps, case["mode"])
    for i in range(maps.shape[0]):
        imgs[f"shadow_maps[{i}]"] = make_image(maps.shape[2], maps.shape[1], fmt, "in", f"shadow_maps[{i}]").upload(maps[i])
        a.shadow_maps[i] = imgs[f"shadow_maps[{i}]"].desc
    flat = np.asarray(case["transforms"], np.float32).reshape(4, 16)
    for i in range(4):
        a.transforms[i][:] = [float(v) for v in flat[i]]
    return a, imgs


def download_rgba16f(image):
    """(h, w, 4) uint16 of an RGBA16F image, whichever class holds it"""
    return np.ascontiguousarray(image.download()).view(np.uint16).reshape(image.height, image.width, 4)


def download_moments(image):
    """(h, w, 2) float32 of an R32G32_SFLOAT image"""
    return np.ascontiguousarray(image.download()).view(np.float32).reshape(image.height, image.width, 2)
