"""CPU: the C ABI of the SSAO entry points without a device.  The host restatement of the constant block gives the bytes the reference's own
ffx_cacao.cpp wrote (tests/golden/cacao_constants_v1.npz); the ctypes structs have the header's layout; every symbol is exported and bound;
the workspace description is consistent; and everything the launchers refuse is refused against the device-less HIP stand-in of
tests/hip_stub with the rule in gr_last_error and a launch count of zero, while the valid calls launch.

Run as a program (the worker of the refusal test, under the stand-in) it prints {case: [code, message, launches]}."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
INVALID, UNSUPPORTED = -1, -3
ENTRY_POINTS = ("gr_cacao_reference_settings", "gr_cacao_update_buffer_sizes", "gr_cacao_update_constants", "gr_cacao_workspace_bytes",
                "gr_cacao_workspace_describe", "gr_cacao_prepare_depths", "gr_cacao_prepare_normals", "gr_cacao_generate_base",
                "gr_cacao_importance_generate", "gr_cacao_importance_postprocess_a", "gr_cacao_importance_postprocess_b", "gr_cacao_generate",
                "gr_cacao_blur", "gr_cacao_apply")


def test_struct_layouts():
    from granite_amd import capi
    import cacao_ref as cr
    c = capi.CacaoConstants
    assert C.sizeof(c) == 384 == cr.CONSTANTS_DTYPE.itemsize
    for name in cr.CONSTANTS_DTYPE.names:
        assert getattr(c, name).offset == cr.CONSTANTS_DTYPE.fields[name][1], name
    assert C.sizeof(capi.CacaoSettings) == 68 and capi.CacaoSettings.quality_level.offset == 28 and capi.CacaoSettings.generate_normals.offset == 56
    assert C.sizeof(capi.CacaoBufferSizes) == 64
    assert C.sizeof(capi.CacaoIntermediate) == 32 + 5 * 4 + 4 + 4 * 8 + 8


def test_entry_points_are_exported_and_bound():
    from granite_amd import capi
    lib = capi.load_library()
    for name in ENTRY_POINTS:
        assert name in capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    with open(os.path.join(ROOT, "include", "granite_hip.h")) as f:
        header = f.read()
    declared = {name for name in ENTRY_POINTS if name + "(" in header}
    assert declared == set(ENTRY_POINTS)


def test_constants_are_the_references_bytes():
    from granite_amd import capi
    import cacao_cases as cc
    import cacao_ref as cr
    g = cc.golden()
    lib = capi.load_library()
    for w, h in cc.SIZES:
        sizes = capi.CacaoBufferSizes()
        assert lib.gr_cacao_update_buffer_sizes(w, h, C.byref(sizes)) == 0
        assert np.array_equal(np.frombuffer(bytes(sizes), np.uint32), g[f"{w}x{h}/sizes"])
        for cam_name in cc.CAMERAS:
            for variant in cc.SETTINGS:
                for quality in cc.QUALITIES:
                    k = cc.key(w, h, cam_name, variant, quality)
                    settings = capi.CacaoSettings.from_buffer_copy(g[k + "/settings"].tobytes())
                    got = np.frombuffer(bytes(capi.cacao_constants(w, h, g[k + "/proj"], g[k + "/view"], settings)), cr.CONSTANTS_DTYPE)
                    want = g[k + "/constants"].view(cr.CONSTANTS_DTYPE).reshape(4)
                    for name in cr.CONSTANTS_DTYPE.names:
                        if name == "PatternRotScaleMatrices":  # cosf / sinf belong to the math library of the day
                            ulps = np.abs(got[name].view(np.int32).astype(np.int64) - want[name].view(np.int32).astype(np.int64))
                            assert ulps.max() <= 1, (k, name)
                        else:
                            assert got[name].tobytes() == want[name].tobytes(), (k, name, got[name], want[name])
    assert bytes(capi.cacao_reference_settings()) == cc.settings_words("reference", cr.QUALITY_HIGHEST).tobytes()


def test_settings_outside_the_configuration_are_refused():
    from granite_amd import capi
    lib = capi.load_library()
    sizes = capi.CacaoBufferSizes()
    lib.gr_cacao_update_buffer_sizes(64, 48, C.byref(sizes))
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    constants = (capi.CacaoConstants * 4)()

    def code(**changes):
        s = capi.cacao_reference_settings()
        for name, value in changes.items():
            setattr(s, name, value)
        return lib.gr_cacao_update_constants(None, constants, C.byref(s), C.byref(sizes), eye, eye)
    assert code() == 0 and code(quality_level=capi.CACAO_QUALITY_HIGH, blur_pass_count=0) == 0 and code(blur_pass_count=8) == 0
    for quality in (0, 1, 2, 5):
        assert code(quality_level=quality) == INVALID
    assert code(generate_normals=1) == INVALID and code(blur_pass_count=9) == INVALID
    downsampled = capi.CacaoBufferSizes.from_buffer_copy(bytes(sizes))
    downsampled.ssaoBufferWidth = 16  # what useDownsampledSsao would give
    assert lib.gr_cacao_update_constants(None, constants, C.byref(capi.cacao_reference_settings()), C.byref(downsampled), eye, eye) == INVALID
    for w, h in ((0, 4), (4, 0), (capi.CACAO_MAX_EXTENT + 1, 4)):
        assert lib.gr_cacao_update_buffer_sizes(w, h, C.byref(sizes)) == INVALID and lib.gr_cacao_workspace_bytes(w, h) == 0
        assert capi.cacao_workspace_describe(w, h) is None


def test_workspace_description():
    from granite_amd import capi
    import cacao_cases as cc
    for w, h in cc.SIZES + ((3840, 2160),):
        d = capi.cacao_workspace_describe(w, h)
        hw, hh = (w + 1) // 2, (h + 1) // 2
        assert [(e["name"], e["format"], e["layers"], e["mips"]) for e in d] == [
            ("FFX_CACAO_DEINTERLEAVED_DEPTHS", capi.FORMAT_R16_SFLOAT, 4, 4), ("FFX_CACAO_DEINTERLEAVED_NORMALS", capi.CACAO_FORMAT_R8G8B8A8_SNORM, 4, 1),
            ("FFX_CACAO_SSAO_BUFFER_PING", capi.FORMAT_R8G8_UNORM, 4, 1), ("FFX_CACAO_SSAO_BUFFER_PONG", capi.FORMAT_R8G8_UNORM, 4, 1),
            ("FFX_CACAO_IMPORTANCE_MAP", capi.FORMAT_R8_UNORM, 1, 1), ("FFX_CACAO_IMPORTANCE_MAP_PONG", capi.FORMAT_R8_UNORM, 1, 1),
            ("FFX_CACAO_LOAD_COUNTER", capi.CACAO_FORMAT_R32_UINT, 1, 1)]
        assert [(e["width"], e["height"]) for e in d[:4]] == [(hw, hh)] * 4 and (d[4]["width"], d[4]["height"]) == ((hw + 1) // 2, (hh + 1) // 2)
        assert d[0]["bytes"] == sum(max(1, hw >> k) * max(1, hh >> k) * 8 for k in range(4))
        assert [d[0]["mip_offset"][k + 1] - d[0]["mip_offset"][k] for k in range(3)] == [max(1, hw >> k) * max(1, hh >> k) * 8 for k in range(3)]
        # no two intermediates share a byte, every one starts at a multiple of 256 and lies inside the workspace
        spans = sorted((e["mip_offset"][0], e["mip_offset"][0] + e["bytes"]) for e in d)
        assert all(a % 256 == 0 for a, _ in spans) and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
        assert spans[-1][1] <= capi.load_library().gr_cacao_workspace_bytes(w, h)


def worker():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from granite_amd import capi
    from granite_amd.capi import Image

    stub = C.CDLL(STUB)
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib, h = gr.lib, gr.handle
    W, H = 64, 48
    eye = np.eye(4, dtype=np.float32).reshape(16)
    proj = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0.001, -1, 0, 0, 0.1, 0], np.float32)
    good = capi.cacao_constants(W, H, proj, eye)
    other = capi.cacao_constants(W + 2, H, proj, eye)
    keep = []

    def buffer(nbytes):
        keep.append(capi.DeviceBuffer(gr, nbytes))
        return keep[-1].ptr

    ws = buffer(lib.gr_cacao_workspace_bytes(W, H) + 512)
    ws += (-ws) % 256
    out = {}

    def counted(name, fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        out[name] = [code, lib.gr_last_error(h).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    def image(fmt, w=W, hgt=H, texel=None):
        texel = texel or capi.FORMAT_BPP[fmt]
        return Image(buffer(w * texel * hgt + 64), w, hgt, w * texel, fmt)

    D32, A2, R8 = capi.FORMAT_D32_SFLOAT, capi.FORMAT_A2B10G10R10_UNORM_PACK32, capi.FORMAT_R8_UNORM
    image_calls = {
        "gr_cacao_prepare_depths": (D32, lambda img, w_=None, c=good: lib.gr_cacao_prepare_depths(h, None, img, w_ if w_ is not None else ws, c)),
        "gr_cacao_prepare_normals": (A2, lambda img, w_=None, c=good: lib.gr_cacao_prepare_normals(h, None, img, w_ if w_ is not None else ws, c)),
        "gr_cacao_apply": (R8, lambda img, w_=None, c=good: lib.gr_cacao_apply(h, None, w_ if w_ is not None else ws, img, c, 1)),
    }
    for name, (fmt, call) in image_calls.items():
        counted(f"{name}:valid", lambda: call(C.byref(image(fmt))))
        counted(f"{name}:null_image", lambda: call(None))
        counted(f"{name}:null_ptr", lambda: call(C.byref(Image(None, W, H, W * capi.FORMAT_BPP[fmt], fmt))))
        counted(f"{name}:format", lambda: call(C.byref(image(capi.FORMAT_R16_SFLOAT, texel=capi.FORMAT_BPP[fmt]))))
        counted(f"{name}:width0", lambda: call(C.byref(Image(buffer(64), 0, H, 64, fmt))))
        short = image(fmt)
        short.pitch_bytes = (W - 1) * capi.FORMAT_BPP[fmt]
        counted(f"{name}:pitch_short", lambda: call(C.byref(short)))
        if capi.FORMAT_BPP[fmt] > 1:
            odd = image(fmt)
            odd.pitch_bytes += 1
            counted(f"{name}:pitch+1", lambda: call(C.byref(odd)))
            off = image(fmt)
            off.ptr += 1
            counted(f"{name}:ptr+1", lambda: call(C.byref(off)))
        counted(f"{name}:size", lambda: call(C.byref(image(fmt, W + 2, H))))  # the constants were made for another size
        counted(f"{name}:too_large", lambda: call(C.byref(Image(buffer(64), capi.CACAO_MAX_EXTENT + 1, 1, (capi.CACAO_MAX_EXTENT + 1) * 4, fmt))))
        counted(f"{name}:null_workspace", lambda: call(C.byref(image(fmt)), 0))
        counted(f"{name}:workspace+64", lambda: call(C.byref(image(fmt)), ws + 64))
        counted(f"{name}:null_constants", lambda: call(C.byref(image(fmt)), None, None))
        counted(f"{name}:other_constants", lambda: call(C.byref(image(fmt)), None, other))
        inside = Image(ws, W, H, W * capi.FORMAT_BPP[fmt], fmt)
        counted(f"{name}:image_in_workspace", lambda: call(C.byref(inside)))

    plain = {
        "gr_cacao_generate_base": lambda w_, wd, hg, c: lib.gr_cacao_generate_base(h, None, w_, wd, hg, c),
        "gr_cacao_importance_generate": lambda w_, wd, hg, c: lib.gr_cacao_importance_generate(h, None, w_, wd, hg, c),
        "gr_cacao_importance_postprocess_a": lambda w_, wd, hg, c: lib.gr_cacao_importance_postprocess_a(h, None, w_, wd, hg, c),
        "gr_cacao_importance_postprocess_b": lambda w_, wd, hg, c: lib.gr_cacao_importance_postprocess_b(h, None, w_, wd, hg, c),
        "gr_cacao_generate": lambda w_, wd, hg, c: lib.gr_cacao_generate(h, None, w_, wd, hg, c, capi.CACAO_QUALITY_HIGHEST),
        "gr_cacao_blur": lambda w_, wd, hg, c: lib.gr_cacao_blur(h, None, w_, wd, hg, c, 2),
    }
    for name, call in plain.items():
        counted(f"{name}:valid", lambda: call(ws, W, H, good))
        counted(f"{name}:null_workspace", lambda: call(None, W, H, good))
        counted(f"{name}:workspace+64", lambda: call(ws + 64, W, H, good))
        counted(f"{name}:null_constants", lambda: call(ws, W, H, None))
        counted(f"{name}:width0", lambda: call(ws, 0, H, good))
        counted(f"{name}:too_large", lambda: call(ws, W, capi.CACAO_MAX_EXTENT + 1, good))
        counted(f"{name}:other_size", lambda: call(ws, W + 2, H, good))
    counted("gr_cacao_generate:valid_high", lambda: lib.gr_cacao_generate(h, None, ws, W, H, good, capi.CACAO_QUALITY_HIGH))
    for quality in (0, 1, 2, 5):
        counted(f"gr_cacao_generate:quality{quality}", lambda: lib.gr_cacao_generate(h, None, ws, W, H, good, quality))
    for passes in (0, 9):
        counted(f"gr_cacao_blur:passes{passes}", lambda: lib.gr_cacao_blur(h, None, ws, W, H, good, passes))
    for passes in (1, 8):
        counted(f"gr_cacao_blur:valid_passes{passes}", lambda: lib.gr_cacao_blur(h, None, ws, W, H, good, passes))
    settings = capi.cacao_reference_settings()
    settings.quality_level = 2
    sizes = capi.CacaoBufferSizes()
    lib.gr_cacao_update_buffer_sizes(W, H, C.byref(sizes))
    four = (capi.CacaoConstants * 4)()
    vec = (C.c_float * 16)(*eye)
    counted("gr_cacao_update_constants:quality2", lambda: lib.gr_cacao_update_constants(h, four, C.byref(settings), C.byref(sizes), vec, vec))
    print(json.dumps(out))


def test_refusals_launch_nothing():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))  # in front of whatever is preloaded already
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    wrong = []
    for case, (code, message, launches) in sorted(got.items()):
        function, what = case.split(":")
        if what.startswith("valid"):
            if code != 0 or launches != 1:
                wrong.append((case, code, message, launches))
            continue
        expected = UNSUPPORTED if what == "format" else INVALID
        if code != expected or launches != 0 or not message.startswith(function + ": ") or len(message) < len(function) + 20:
            wrong.append((case, code, message, launches))
    assert not wrong, wrong
    assert sum(1 for case in got if case.split(":")[1].startswith("valid")) == 12 and len(got) > 90
    # the rule is named
    assert "256-byte aligned" in got["gr_cacao_blur:workspace+64"][1]
    assert "pitch_bytes" in got["gr_cacao_prepare_depths:pitch+1"][1] and "depth" in got["gr_cacao_prepare_depths:pitch+1"][1]
    assert "overlaps" in got["gr_cacao_apply:image_in_workspace"][1]
    assert "not made for this width and height" in got["gr_cacao_generate:other_size"][1]
    assert "quality" in got["gr_cacao_generate:quality2"][1] and "1 .. 8" in got["gr_cacao_blur:passes0"][1]
    assert "quality_level" in got["gr_cacao_update_constants:quality2"][1]


if __name__ == "__main__":
    worker()
