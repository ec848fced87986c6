"""CPU: images whose last byte lies 4 GiB or more behind their pointer, against the device-less HIP stand-in of tests/hip_stub.

The kernels of gr_lighting and of the anti-aliasing launchers (aa.hip: FXAA, the three SMAA passes, the TAA resolve, the blit) form
`y * pitch_bytes + x * texel` in 32 bits, so each of their image arguments is refused with GR_ERR_INVALID_ARGUMENT, by name and without a
launch, when pitch_bytes * height is above 2^32 - 1 (image_args.hpp: gr_image_offset_rule; stated at the entry points in granite_hip.h) --
an attachment viewed out of a large atlas is such an image.  The same call with the image 16 bytes short of 4 GiB launches.  The launchers whose kernels
form the offset in 64 bits take such an image: one case each shows that they launch.

Where a row offset is formed in 32 bits (`uint32_t(y) * pitch`, `uy * a.X.pitch`), and the answer at each site -- a refusal at the entry point,
so that no compiled kernel changes:

    lighting.hip    load_raw: depth, albedo, normal, pbr, emissive; shade_tile's store: hdr      gr_lighting, each of the six attachments
    aa.hip          Tex8::fetch (k_fxaa_generic, k_smaa_edges_generic, k_smaa_blend_generic)      gr_fxaa, gr_smaa_edge_detection, gr_smaa_neighbor_blend
    aa.hip          blit_texel's RGBA8 fetch, k_blit's RGBA8 store                                gr_blit: in, out
    aa_fast_kernels.hpp  load_rgba8_clamped, k_fxaa_fast, k_smaa_edges_fast, k_smaa_blend_fast     gr_fxaa: in, out; edge detection: color, edges; blend: color, weights, out
    aa_fast_kernels.hpp  k_taa_fast, taa_load_current, TaaMotion, TaaHistory                      gr_taa_resolve: current, depth, mv, history, out_color, out_history
    smaa_weights.hpp     k_smaa_pack_edges, k_smaa_weights_bits                                   gr_smaa_blend_weight: edges, weights

post.hip, fsr.hip, hdr10.hip, hiz.hip, spd.hip, ssr.hip, decal.hip, ocean.hip, environment.hip and device_common.hpp widen y to size_t first.

Every image is 16 x 5, so only the pitch of the argument under test moves: 5 * 858993464 = 2^32 + 24, 5 * 858993456 = 2^32 - 16.  The pointers
are made up, distinct, 256-byte aligned and 64 GiB apart; nothing is dereferenced, and none of these cases may run on a device.

Run as a program (the worker of the test) it prints {case: [code, message, launches]}."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
INVALID = -1
W, H = 16, 5
ABOVE, BELOW = 858993464, 858993456  # multiples of 8 and of every texel size
assert ABOVE * H > 0xffffffff >= BELOW * H and ABOVE % 8 == 0 and BELOW % 8 == 0 and ABOVE < 1 << 32


def worker():
    sys.path.insert(0, ROOT)
    from granite_amd import capi
    from granite_amd.capi import Image

    stub = C.CDLL(STUB)
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib = gr.lib
    RGBA8, SRGB8, RG8, R8 = capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8B8A8_SRGB, capi.FORMAT_R8G8_UNORM, capi.FORMAT_R8_UNORM
    H4, H2, H1, B10 = capi.FORMAT_R16G16B16A16_SFLOAT, capi.FORMAT_R16G16_SFLOAT, capi.FORMAT_R16_SFLOAT, capi.FORMAT_B10G11R11_UFLOAT_PACK32
    D32, A2 = capi.FORMAT_D32_SFLOAT, capi.FORMAT_A2B10G10R10_UNORM_PACK32
    scratch = capi.DeviceBuffer(gr, 1 << 20)  # the non-image arguments: real, never written by the stand-in
    made = [0]

    def fake_ptr():
        made[0] += 1
        return 0x1000_0000_0000 + (made[0] << 36)

    def ref(img):
        return C.byref(img) if img is not None else None

    def counted(fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        return [code, lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    out = {}

    def images_of(spec, pitches):
        return {arg: Image(fake_ptr(), w, h, pitches.get(arg, w * capi.FORMAT_BPP[fmt]), fmt) for arg, (w, h, fmt) in spec.items()}

    def narrow(name, spec, call, optional=()):
        """An entry point whose kernels form offsets in 32 bits: each argument in turn above and below the limit."""
        out[f"{name}:tight"] = counted(lambda: call(images_of(spec, {})))
        for arg in spec:
            out[f"{name}:above:{arg}"] = counted(lambda: call(images_of(spec, {arg: ABOVE})))
            out[f"{name}:below:{arg}"] = counted(lambda: call(images_of(spec, {arg: BELOW})))
        out[f"{name}:below_all"] = counted(lambda: call(images_of(spec, dict.fromkeys(spec, BELOW))))
        for arg in optional:
            def without(arg=arg):
                images = images_of(spec, dict.fromkeys(spec, BELOW))
                images[arg] = None
                return call(images)
            out[f"{name}:below_all_without:{arg}"] = counted(without)

    def wide(name, spec, call, tight=()):
        """An entry point whose kernels form offsets in 64 bits: every argument above the limit at once (but those documented as tight)."""
        out[f"{name}:wide_above_all"] = counted(lambda: call(images_of(spec, {arg: ABOVE for arg in spec if arg not in tight})))

    S = (W, H)
    # ---- lighting.hip ---------------------------------------------------------------------------------------------------------
    def lighting(I, fmt=H4, flags=capi.LIGHTING_DIRECTIONAL_BIT, alias=False):
        a = capi.LightingArgs()
        for arg in ("hdr", "emissive", "albedo", "normal", "pbr", "depth"):
            setattr(a, arg, I["hdr" if alias and arg == "emissive" else arg])
        if "ambient_occlusion" in I:
            a.ambient_occlusion = I["ambient_occlusion"]
        a.flags = flags
        return lib.gr_lighting(gr.handle, None, C.byref(a))
    for tag, fmt in (("", H4), ("_b10g11r11", B10)):
        gbuffer = {"hdr": (*S, fmt), "emissive": (*S, fmt), "albedo": (*S, SRGB8), "normal": (*S, A2), "pbr": (*S, RG8), "depth": (*S, D32)}
        narrow("gr_lighting" + tag, gbuffer, lighting)
    aliased = {arg: size for arg, size in gbuffer.items() if arg != "emissive"}
    narrow("gr_lighting_aliased", aliased, lambda I: lighting(I, alias=True))
    # the ambient-occlusion image is sampled through 64-bit offsets: no limit of its own
    with_ao = dict(gbuffer, ambient_occlusion=(8, 5, R8))
    ao_flags = capi.LIGHTING_DIRECTIONAL_BIT | capi.LIGHTING_AMBIENT_FALLBACK_BIT | capi.LIGHTING_AMBIENT_OCCLUSION_BIT
    out["gr_lighting:wide_above:ambient_occlusion"] = counted(lambda: lighting(images_of(with_ao, {"ambient_occlusion": ABOVE}), flags=ao_flags))

    # ---- aa.hip ---------------------------------------------------------------------------------------------------------------
    fxaa, smaa = capi.PushFxaa((1 / W, 1 / H)), capi.PushSmaa((1 / W, 1 / H, W, H))
    taa = capi.PushTaa()
    lib.gr_smaa_set_luts(gr.handle, bytes(160 * 560 * 2), bytes(64 * 16))
    narrow("gr_fxaa", {"in": (*S, SRGB8), "out": (*S, RGBA8)}, lambda I: lib.gr_fxaa(gr.handle, None, ref(I["in"]), ref(I["out"]), C.byref(fxaa)))
    narrow("gr_smaa_edge_detection", {"color": (*S, SRGB8), "edges": (*S, RG8)},
           lambda I: lib.gr_smaa_edge_detection(gr.handle, None, ref(I["color"]), ref(I["edges"]), C.byref(smaa), 2))
    narrow("gr_smaa_blend_weight", {"edges": (*S, RG8), "weights": (*S, RGBA8)},
           lambda I: lib.gr_smaa_blend_weight(gr.handle, None, ref(I["edges"]), ref(I["weights"]), C.byref(smaa), 2))
    narrow("gr_smaa_neighbor_blend", {"color": (*S, SRGB8), "weights": (*S, RGBA8), "out": (*S, SRGB8)},
           lambda I: lib.gr_smaa_neighbor_blend(gr.handle, None, ref(I["color"]), ref(I["weights"]), ref(I["out"]), C.byref(smaa)))
    for tag, fmt in (("", H4), ("_b10g11r11", B10)):
        narrow("gr_taa_resolve" + tag, {"current": (*S, fmt), "depth": (*S, D32), "mv": (*S, H2), "history": (*S, H4), "out_color": (*S, fmt), "out_history": (*S, H4)},
               lambda I: lib.gr_taa_resolve(gr.handle, None, ref(I["current"]), ref(I["depth"]), ref(I["mv"]), ref(I["history"]), ref(I["out_color"]),
                                            ref(I["out_history"]), C.byref(taa), 1), optional=["history"] if not tag else [])
    narrow("gr_blit", {"in": (*S, SRGB8), "out": (32, H, RGBA8)}, lambda I: lib.gr_blit(gr.handle, None, ref(I["in"]), ref(I["out"]), 1))
    narrow("gr_blit_rgba16f", {"in": (*S, H4), "out": (32, H, H4)}, lambda I: lib.gr_blit(gr.handle, None, ref(I["in"]), ref(I["out"]), 0))

    # ---- 64-bit offsets throughout: post.hip, fsr.hip, hdr10.hip, hiz.hip, spd.hip, ssr.hip -----------------------------------------
    half, quarter = (8, 3), (4, 2)
    wide("gr_bloom_threshold", {"hdr": (*S, H4), "out": (*half, H4)},
         lambda I: lib.gr_bloom_threshold(gr.handle, None, ref(I["hdr"]), ref(I["out"]), None, C.byref(capi.threshold_push(I["out"]))))
    wide("gr_bloom_downsample", {"in": (*S, H4), "out": (*half, H4), "history": (*half, H4)},
         lambda I: lib.gr_bloom_downsample(gr.handle, None, ref(I["in"]), ref(I["out"]), ref(I["history"]), C.byref(capi.downsample_push(I["out"], I["in"], 0.5))))
    wide("gr_bloom_upsample", {"in": (*half, H4), "out": (*S, H4)},
         lambda I: lib.gr_bloom_upsample(gr.handle, None, ref(I["in"]), ref(I["out"]), C.byref(capi.upsample_push(I["out"], I["in"]))))
    wide("gr_tonemap", {"hdr": (*S, H4), "bloom": (*quarter, H4), "out": (*S, SRGB8)},
         lambda I: lib.gr_tonemap(gr.handle, None, ref(I["hdr"]), ref(I["bloom"]), ref(I["out"]), None, C.byref(capi.PushTonemap(1.0))))
    wide("gr_fsr_upscale", {"in": (*S, SRGB8), "out": (32, H, SRGB8)}, lambda I: lib.gr_fsr_upscale(gr.handle, None, ref(I["in"]), ref(I["out"]), 0))
    wide("gr_fsr_sharpen", {"in": (*S, SRGB8), "out": (*S, SRGB8)}, lambda I: lib.gr_fsr_sharpen(gr.handle, None, ref(I["in"]), ref(I["out"]), C.c_float(0.5)))
    pq = capi.PushPq10()
    pq.max_light_level, pq.inv_max_light_level = 1000.0, 0.001
    wide("gr_pq10_encode", {"hdr": (*S, H4), "ui": (*S, SRGB8), "out": (*S, A2)},
         lambda I: lib.gr_pq10_encode(gr.handle, None, ref(I["hdr"]), ref(I["ui"]), ref(I["out"]), C.byref(pq)))

    def hiz(I):
        a = capi.HizArgs()
        a.depth, a.chain, a.chain_width, a.chain_height, a.chain_levels, a.counter = I["depth"], scratch.ptr, 64, 64, 1, scratch.ptr
        return lib.gr_hiz(gr.handle, None, C.byref(a))
    wide("gr_hiz", {"depth": (*S, D32)}, hiz)

    def spd(I):
        a = capi.SpdArgs(I["input"], scratch.ptr, 8, 4, 2, 4, capi.SPD_REDUCTION_COLOR, None)
        return lib.gr_spd_downsample(gr.handle, None, C.byref(a))
    wide("gr_spd_downsample", {"input": (*S, H4)}, spd)
    trace = {"output": (*S, H4), "ray_length": (*S, H1), "ray_confidence": (*S, R8), "light": (*S, H4), "normal": (*S, A2), "pbr": (*S, RG8)}

    def ssr_trace(I):
        a = capi.SsrArgs()
        for arg in trace:
            setattr(a, arg, I[arg])
        a.depth_chain, a.chain_width, a.chain_height, a.chain_levels = scratch.ptr, 16, 8, 1
        a.dither_lut = a.ray_list = a.ray_counter = a.scratch = scratch.ptr
        return lib.gr_ssr_trace(gr.handle, None, C.byref(a))
    wide("gr_ssr_trace", trace, ssr_trace)
    apply = {"hdr": (*S, H4), "reflected": (*S, H4), "albedo": (*S, SRGB8), "normal": (*S, A2), "pbr": (*S, RG8), "depth": (*S, D32), "brdf_lut": (4, 2, H2)}

    def ssr_apply(I):
        a = capi.SsrApplyArgs()
        for arg in apply:
            setattr(a, arg, I[arg])
        return lib.gr_ssr_apply(gr.handle, None, C.byref(a))
    wide("gr_ssr_apply", apply, ssr_apply, tight=["brdf_lut"])  # (the table is indexed without a pitch: ssr.hip, stated at gr_ssr_apply)
    print(json.dumps(out))


def run_worker():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))  # in front of whatever is preloaded already
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


NARROW = {"gr_lighting": 6, "gr_lighting_b10g11r11": 6, "gr_lighting_aliased": 5, "gr_fxaa": 2, "gr_smaa_edge_detection": 2, "gr_smaa_blend_weight": 2,
          "gr_smaa_neighbor_blend": 3, "gr_taa_resolve": 6, "gr_taa_resolve_b10g11r11": 6, "gr_blit": 2, "gr_blit_rgba16f": 2}
LAUNCHES = {"gr_smaa_blend_weight": 2}  # the edges packed into bit planes, then the weights
WIDE = ("gr_bloom_threshold", "gr_bloom_downsample", "gr_bloom_upsample", "gr_tonemap", "gr_fsr_upscale", "gr_fsr_sharpen", "gr_pq10_encode", "gr_hiz",
        "gr_spd_downsample", "gr_ssr_trace", "gr_ssr_apply")


def test_images_past_4_gib_are_refused_by_name_where_offsets_are_32_bit_and_taken_elsewhere():
    got = run_worker()
    wrong = []
    seen = {name: 0 for name in NARROW}
    for case, (code, message, launches) in sorted(got.items()):
        name, what, *rest = case.split(":")
        if what == "above":
            argument = rest[0]
            seen[name] += 1
            named = re.search(rf"(?<![A-Za-z0-9_]){argument} pitch_bytes \* height is above 4 GiB", message) is not None
            entry_point = name.replace("_b10g11r11", "").replace("_aliased", "").replace("_rgba16f", "")
            if code != INVALID or launches != 0 or not named or not message.startswith(entry_point):
                wrong.append((case, "not refused by name without a launch", code, message, launches))
        elif what.startswith("wide_above"):
            if code != 0 or launches < 1:
                wrong.append((case, "a launcher with 64-bit offsets must take the image", code, message, launches))
        else:  # tight, below:<argument>, below_all, below_all_without:<argument>
            if code != 0 or launches != LAUNCHES.get(name, 1):
                wrong.append((case, "a call within the limit must launch", code, message, launches))
    assert not wrong, wrong
    assert seen == NARROW, seen
    for name, arguments in NARROW.items():
        assert sum(case.startswith(name + ":below:") for case in got) == arguments and f"{name}:below_all" in got and f"{name}:tight" in got
    assert "gr_taa_resolve:below_all_without:history" in got and "gr_lighting:wide_above:ambient_occlusion" in got
    assert all(f"{name}:wide_above_all" in got for name in WIDE)


if __name__ == "__main__":
    worker()
