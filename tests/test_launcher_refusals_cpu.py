"""CPU: what every launcher of the C ABI does with a malformed gr_image (granite_amd/csrc/image_args.hpp), against the device-less HIP
stand-in of tests/hip_stub: the returned code, the message, and the number of launches, per entry point and per way an image can be wrong.

The table was run once against the libraries of the commit before the launchers shared one contract; that column is
tests/golden/launcher_refusals_parent.json ({case: [code, launches]}).  A row tagged T1..T4 is one of the four tightenings the shared contract
brought -- pitch_bytes (T1) or ptr (T2) not a multiple of the texel size, a row cover that only held in 32 bits (T3), an output that shares bytes
with its input other than by an equal pointer (T4): it must be refused with GR_ERR_INVALID_ARGUMENT, launch nothing and name the argument.
Every other row must do what the parent did, code and launches; a refusal launches nothing.  gr_video_scale, gr_video_yuv_to_rgb and
gr_texture_decode address single bytes and take an image at any alignment: their pitch + 1 and pointer + 1 rows are untagged.

These cases exist here only: each describes memory that a kernel must not touch, so none of them may run on a device.

Run as a program (the worker of the test; GRANITE_LIB_DIR selects the libraries) it prints {case: [code, message, launches]}."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
PARENT = os.path.join(ROOT, "tests", "golden", "launcher_refusals_parent.json")
INVALID = -1
WRAP = {4: 0x40000001, 8: 0x20000001, 2: 0x80000001}  # width * texel bytes = 2^32 (2^33) + texel bytes: inside a 16-texel pitch in 32 bits


def worker():
    sys.path.insert(0, ROOT)
    from granite_amd import capi
    from granite_amd.capi import Image

    stub = C.CDLL(STUB)
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib = gr.lib
    vp, P = C.c_void_p, C.POINTER
    lib.gr_pack_rgb8_rows.argtypes = [vp, vp, P(Image), P(capi.Rows), vp]
    lib.gr_unpack_rgb8_rows.argtypes = [vp, vp, vp, P(Image), P(capi.Rows)]
    lib.gr_fft_execute.argtypes = [vp, vp, vp, P(capi.FftResource), P(capi.FftResource)]

    RGBA8, SRGB8, RG8, R8 = capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8B8A8_SRGB, capi.FORMAT_R8G8_UNORM, capi.FORMAT_R8_UNORM
    H4, H2, H1 = capi.FORMAT_R16G16B16A16_SFLOAT, capi.FORMAT_R16G16_SFLOAT, capi.FORMAT_R16_SFLOAT
    D32, A2 = capi.FORMAT_D32_SFLOAT, capi.FORMAT_A2B10G10R10_UNORM_PACK32
    WRONG = capi.FORMAT_D16_UNORM  # no launcher takes it
    keep = []  # device buffers stay allocated for the run

    def buffer(nbytes):
        keep.append(capi.DeviceBuffer(gr, nbytes))
        return keep[-1].ptr

    def ref(img):
        return C.byref(img) if img is not None else None

    def counted(fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        return [code, lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    out = {}

    def entry(name, images, call, pairs=(), embedded=(), byte_addressed=False, in_place=()):
        """images: {argument: (width, height, format)}, the first one sets the size of the call; call(I) with I = {argument: Image or None};
        pairs: (output, input) that must not share bytes; embedded: arguments that are no pointers (no null image); in_place: (a, b) that
        may be the same image."""
        def fresh():
            made = {}
            for arg, (w, h, fmt) in images.items():
                pitch = w * capi.FORMAT_BPP[fmt]
                made[arg] = Image(buffer(2 * pitch * (h + 1) + 512), w, h, pitch, fmt)
            return made

        def case(what, change):
            I = fresh()
            change(I)
            out[f"{name}:{what}"] = counted(lambda: call(I))

        first = next(iter(images))
        case("valid", lambda I: None)
        for arg, (w, h, fmt) in images.items():
            texel = capi.FORMAT_BPP[fmt]
            if arg not in embedded:
                case(f"null_image:{arg}", lambda I: I.__setitem__(arg, None))
            case(f"null_ptr:{arg}", lambda I: setattr(I[arg], "ptr", None))
            case(f"format:{arg}", lambda I: setattr(I[arg], "format", WRONG))
            case(f"width0:{arg}", lambda I: setattr(I[arg], "width", 0))
            if arg != first:
                case(f"size:{arg}", lambda I: setattr(I[arg], "height", h + 1))
            case(f"pitch_short:{arg}", lambda I: setattr(I[arg], "pitch_bytes", (w - 1) * texel))
            if texel > 1:
                tag = "" if byte_addressed else "T1 "
                case(f"{tag}pitch+1:{arg}", lambda I: setattr(I[arg], "pitch_bytes", w * texel + 1))
                tag = "" if byte_addressed else "T2 "
                case(f"{tag}ptr+1:{arg}", lambda I: setattr(I[arg], "ptr", I[arg].ptr + 1))
                case(f"T3 wrap:{arg}", lambda I: setattr(I[arg], "width", WRAP[texel]))
        texel = capi.FORMAT_BPP[images[first][2]]
        if texel > 1:
            def wrap_all(I):
                for img in I.values():
                    img.width = WRAP[texel]
            case(f"T3 wrap_all:{first}", wrap_all)
        for a, b in pairs:
            case(f"T4 row_into:{a}<{b}", lambda I: setattr(I[a], "ptr", I[b].ptr + I[b].pitch_bytes))
            case(f"equal:{a}={b}", lambda I: setattr(I[a], "ptr", I[b].ptr))
        for a, b in in_place:
            case(f"in_place:{a}={b}", lambda I: setattr(I[a], "ptr", I[b].ptr))

    S = 16, 8
    half, quarter, eighth, double = (8, 4), (4, 2), (2, 1), (32, 16)
    scratch = buffer(1 << 20)

    # ---- aa.hip ---------------------------------------------------------------------------------------------------------------
    fxaa, smaa = capi.PushFxaa((1 / 16, 1 / 8)), capi.PushSmaa((1 / 16, 1 / 8, 16, 8))
    taa = capi.PushTaa()
    lib.gr_smaa_set_luts(gr.handle, bytes(160 * 560 * 2), bytes(64 * 16))
    entry("gr_fxaa", {"in": (*S, SRGB8), "out": (*S, RGBA8)}, lambda I: lib.gr_fxaa(gr.handle, None, ref(I["in"]), ref(I["out"]), C.byref(fxaa)),
          pairs=[("out", "in")])
    entry("gr_smaa_edge_detection", {"color": (*S, SRGB8), "edges": (*S, RG8)},
          lambda I: lib.gr_smaa_edge_detection(gr.handle, None, ref(I["color"]), ref(I["edges"]), C.byref(smaa), 2))
    entry("gr_smaa_blend_weight", {"edges": (*S, RG8), "weights": (*S, RGBA8)},
          lambda I: lib.gr_smaa_blend_weight(gr.handle, None, ref(I["edges"]), ref(I["weights"]), C.byref(smaa), 2))
    entry("gr_smaa_neighbor_blend", {"color": (*S, SRGB8), "weights": (*S, RGBA8), "out": (*S, SRGB8)},
          lambda I: lib.gr_smaa_neighbor_blend(gr.handle, None, ref(I["color"]), ref(I["weights"]), ref(I["out"]), C.byref(smaa)), pairs=[("out", "color")])
    entry("gr_taa_resolve", {"current": (*S, H4), "depth": (*S, D32), "mv": (*S, H2), "history": (*S, H4), "out_color": (*S, H4), "out_history": (*S, H4)},
          lambda I: lib.gr_taa_resolve(gr.handle, None, ref(I["current"]), ref(I["depth"]), ref(I["mv"]), ref(I["history"]), ref(I["out_color"]),
                                       ref(I["out_history"]), C.byref(taa), 1), pairs=[("out_history", "history")])
    entry("gr_blit", {"in": (*S, H4), "out": (*double, SRGB8)}, lambda I: lib.gr_blit(gr.handle, None, ref(I["in"]), ref(I["out"]), 1), pairs=[("out", "in")])

    # ---- post.hip -------------------------------------------------------------------------------------------------------------
    entry("gr_bloom_threshold", {"hdr": (*S, H4), "out": (*half, H4)},
          lambda I: lib.gr_bloom_threshold(gr.handle, None, ref(I["hdr"]), ref(I["out"]), None, C.byref(capi.PushBloomThreshold(half, (1 / 8, 1 / 4)))))
    entry("gr_bloom_downsample", {"in": (*S, H4), "out": (*half, H4), "history": (*half, H4)},
          lambda I: lib.gr_bloom_downsample(gr.handle, None, ref(I["in"]), ref(I["out"]), ref(I["history"]),
                                            C.byref(capi.PushBloomDownsample(half, (1 / 8, 1 / 4), (1 / 16, 1 / 8), 0.5))), pairs=[("history", "out")])
    entry("gr_bloom_upsample", {"in": (*half, H4), "out": (*S, H4)},
          lambda I: lib.gr_bloom_upsample(gr.handle, None, ref(I["in"]), ref(I["out"]), C.byref(capi.PushBloomUpsample(S, (1 / 16, 1 / 8), (1 / 8, 1 / 4)))))
    down = lambda o, i, lerp=0.0: capi.PushBloomDownsample(o, (1 / o[0], 1 / o[1]), (1 / i[0], 1 / i[1]), lerp)
    up = lambda o, i: capi.PushBloomUpsample(o, (1 / o[0], 1 / o[1]), (1 / i[0], 1 / i[1]))
    entry("gr_bloom_down_mid", {"threshold": (*S, H4), "d0": (*half, H4), "d1": (*quarter, H4)},
          lambda I: lib.gr_bloom_down_mid(gr.handle, None, ref(I["threshold"]), ref(I["d0"]), ref(I["d1"]), C.byref(down(half, S)), C.byref(down(quarter, half)), None),
          pairs=[("d1", "d0"), ("d0", "threshold")])
    entry("gr_bloom_down_head", {"hdr": (*double, H4), "threshold": (*S, H4), "d0": (*half, H4), "d1": (*quarter, H4)},
          lambda I: lib.gr_bloom_down_head(gr.handle, None, ref(I["hdr"]), ref(I["threshold"]), ref(I["d0"]), ref(I["d1"]), None,
                                           C.byref(capi.PushBloomThreshold(S, (1 / 16, 1 / 8))), C.byref(down(half, S)), C.byref(down(quarter, half))),
          pairs=[("threshold", "hdr"), ("d0", "threshold"), ("d1", "d0")])
    entry("gr_bloom_down_tail", {"d1": (*S, H4), "d2": (*half, H4), "d3": (*quarter, H4), "history": (*quarter, H4)},
          lambda I: lib.gr_bloom_down_tail(gr.handle, None, ref(I["d1"]), ref(I["d2"]), ref(I["d3"]), ref(I["history"]), C.byref(down(half, S, 0.5)),
                                           C.byref(down(quarter, half, 0.5))), pairs=[("history", "d3")])
    entry("gr_bloom_up_tail", {"d3": (*quarter, H4), "u2": (*half, H4), "u1": (*S, H4)},
          lambda I: lib.gr_bloom_up_tail(gr.handle, None, ref(I["d3"]), ref(I["u2"]), ref(I["u1"]), None, C.byref(up(half, quarter)), C.byref(up(S, half)), None))
    entry("gr_bloom_up_all", {"d3": (*quarter, H4), "u2": (*half, H4), "u1": (*S, H4), "u0": (*double, H4)},
          lambda I: lib.gr_bloom_up_all(gr.handle, None, ref(I["d3"]), ref(I["u2"]), ref(I["u1"]), ref(I["u0"]), None, C.byref(up(half, quarter)),
                                        C.byref(up(S, half)), C.byref(up(double, S)), None, 0), pairs=[("u0", "u1"), ("u1", "u2"), ("u2", "d3")])
    levels = {"hdr": (64, 32), "threshold": double, "d0": S, "d1": half, "d2": quarter, "d3": eighth, "u2": quarter, "u1": half, "u0": S, "history": eighth}

    def pyramid(I):
        a = capi.BloomPyramidArgs()
        for arg in levels:
            setattr(a, arg, I[arg])
        a.push_threshold = capi.PushBloomThreshold(double, (1 / 32, 1 / 16))
        a.push_d0, a.push_d1, a.push_d2, a.push_d3 = down(S, double), down(half, S), down(quarter, half, 0.5), down(eighth, quarter, 0.5)
        a.push_u2, a.push_u1, a.push_u0 = up(quarter, eighth), up(half, quarter), up(S, half)
        return lib.gr_bloom_pyramid(gr.handle, None, C.byref(a))
    entry("gr_bloom_pyramid", {arg: (*size, H4) for arg, size in levels.items()}, pyramid, embedded=list(levels), pairs=[("d0", "threshold"), ("u0", "u1")])
    lum = capi.PushLuminance(S, 0.5, -3.0, 2.0)
    entry("gr_luminance", {"in": (*S, H4)}, lambda I: lib.gr_luminance(gr.handle, None, ref(I["in"]), scratch, C.byref(lum)))
    entry("gr_tonemap", {"hdr": (*S, H4), "bloom": (*quarter, H4), "out": (*S, SRGB8)},
          lambda I: lib.gr_tonemap(gr.handle, None, ref(I["hdr"]), ref(I["bloom"]), ref(I["out"]), None, C.byref(capi.PushTonemap(1.0))))

    # ---- lighting.hip, ssr.hip ------------------------------------------------------------------------------------------------
    gbuffer = {"hdr": (*S, H4), "emissive": (*S, H4), "albedo": (*S, SRGB8), "normal": (*S, A2), "pbr": (*S, RG8), "depth": (*S, D32)}

    def lighting(I, rows=(0, 0)):
        a = capi.LightingArgs()
        for arg in gbuffer:
            setattr(a, arg, I[arg])
        a.flags = capi.LIGHTING_DIRECTIONAL_BIT
        a.rows[:] = rows
        return lib.gr_lighting(gr.handle, None, C.byref(a))
    entry("gr_lighting", gbuffer, lighting, embedded=list(gbuffer), in_place=[("emissive", "hdr")])
    target = {arg: Image(buffer(4096), *S, S[0] * capi.FORMAT_BPP[fmt], fmt) for arg, (_, _, fmt) in gbuffer.items()}
    for rows in ((0, 0), (4, 2), (6, 100), (8, 1)):  # the whole target, a band, a band clipped at the last row, an empty band below it
        out[f"gr_lighting:rows{{{rows[0]}, {rows[1]}}}"] = counted(lambda: lighting(target, rows))

    trace = {"output": (*S, H4), "ray_length": (*S, H1), "ray_confidence": (*S, R8), "light": (*S, H4), "normal": (*S, A2), "pbr": (*S, RG8)}

    def ssr_trace(I):
        a = capi.SsrArgs()
        for arg in trace:
            setattr(a, arg, I[arg])
        a.depth_chain, a.chain_width, a.chain_height, a.chain_levels = scratch, 16, 8, 1
        a.dither_lut = a.ray_list = a.ray_counter = a.scratch = scratch
        return lib.gr_ssr_trace(gr.handle, None, C.byref(a))
    entry("gr_ssr_trace", trace, ssr_trace, embedded=list(trace))
    apply = {"hdr": (*S, H4), "reflected": (*S, H4), "albedo": (*S, SRGB8), "normal": (*S, A2), "pbr": (*S, RG8), "depth": (*S, D32), "brdf_lut": (*quarter, H2)}

    def ssr_apply(I):
        a = capi.SsrApplyArgs()
        for arg in apply:
            setattr(a, arg, I[arg])
        return lib.gr_ssr_apply(gr.handle, None, C.byref(a))
    entry("gr_ssr_apply", apply, ssr_apply, embedded=list(apply))

    # ---- fsr.hip, ctx.hip, spd.hip, hiz.hip, hdr10.hip ---------------------------------------------------------------------------
    entry("gr_fsr_upscale", {"in": (*S, SRGB8), "out": (*double, SRGB8)}, lambda I: lib.gr_fsr_upscale(gr.handle, None, ref(I["in"]), ref(I["out"]), 0),
          pairs=[("out", "in")])
    entry("gr_fsr_sharpen", {"in": (*S, SRGB8), "out": (*S, SRGB8)}, lambda I: lib.gr_fsr_sharpen(gr.handle, None, ref(I["in"]), ref(I["out"]), 0.5),
          pairs=[("out", "in")])
    entry("gr_pack_rgb8_rows", {"image": (*S, SRGB8)}, lambda I: lib.gr_pack_rgb8_rows(gr.handle, None, ref(I["image"]), None, scratch))
    entry("gr_unpack_rgb8_rows", {"image": (*S, SRGB8)}, lambda I: lib.gr_unpack_rgb8_rows(gr.handle, None, scratch, ref(I["image"]), None))

    def spd(I):
        a = capi.SpdArgs(I["input"], scratch, 8, 4, 2, 4, capi.SPD_REDUCTION_COLOR, None)
        return lib.gr_spd_downsample(gr.handle, None, C.byref(a))
    entry("gr_spd_downsample", {"input": (*S, H4)}, spd, embedded=["input"])

    def hiz(I):
        a = capi.HizArgs()
        a.depth, a.chain, a.chain_width, a.chain_height, a.chain_levels, a.counter = I["depth"], scratch, 64, 64, 1, scratch
        return lib.gr_hiz(gr.handle, None, C.byref(a))
    entry("gr_hiz", {"depth": (*S, D32)}, hiz, embedded=["depth"])
    pq = capi.PushPq10()
    pq.max_light_level, pq.inv_max_light_level = 1000.0, 0.001
    entry("gr_pq10_encode", {"hdr": (*S, H4), "ui": (*S, SRGB8), "out": (*S, A2)},
          lambda I: lib.gr_pq10_encode(gr.handle, None, ref(I["hdr"]), ref(I["ui"]), ref(I["out"]), C.byref(pq)))

    # ---- video.hip, ocean.hip, environment.hip, texture_decode.hip, fft.hip ---------------------------------------------------------
    def planes_of(I):
        return (Image * 2)(I["luma"] if "luma" in I else I["output"], I["chroma"])
    srgb = capi.COLOR_SPACE_SRGB_NONLINEAR
    entry("gr_video_scale", {"input": (*S, RGBA8), "output": (*S, R8), "chroma": (*half, RG8)},  # planes[0] is "output" in this entry point's messages
          lambda I: lib.gr_video_scale(gr.handle, None, ref(I["input"]), planes_of(I), 2, srgb, srgb), embedded=["output", "chroma"], byte_addressed=True)
    info = capi.video_yuv_info(full_range=1)
    entry("gr_video_yuv_to_rgb", {"luma": (*S, R8), "chroma": (*half, RG8), "output": (*S, RGBA8)},  # `out`, "output" in this entry point's messages
          lambda I: lib.gr_video_yuv_to_rgb(gr.handle, None, planes_of(I), 2, ref(I["output"]), C.byref(info)), embedded=["luma", "chroma"], byte_addressed=True)
    bake = capi.PushOceanBake((1 / 16, 1 / 8, 1 / 16, 1 / 8), (1.0, 1.0, 1.0, 1.0))
    entry("gr_ocean_bake_maps", {"height": (*S, H1), "displacement": (*S, H2), "grad_jacobian": (*S, H4), "height_displacement": (*S, H4)},
          lambda I: lib.gr_ocean_bake_maps(gr.handle, None, ref(I["height"]), ref(I["displacement"]), ref(I["grad_jacobian"]), ref(I["height_displacement"]),
                                           C.byref(bake)), pairs=[("grad_jacobian", "height"), ("height_displacement", "grad_jacobian")])
    mip = capi.PushOceanMipmap((1.0, 1.0, 1.0, 1.0), (1 / 16, 1 / 8), half, 0.0)
    entry("gr_ocean_mipmap", {"in": (*S, H4), "out": (*half, H4)}, lambda I: lib.gr_ocean_mipmap(gr.handle, None, ref(I["in"]), ref(I["out"]), C.byref(mip)),
          pairs=[("out", "in")])
    cube = buffer(1 << 16)
    entry("gr_env_equirect_to_cube", {"equirect": (*S, H4)}, lambda I: lib.gr_env_equirect_to_cube(gr.handle, None, ref(I["equirect"]), cube, 5, 3))
    entry("gr_texture_decode", {"output": (*S, RGBA8)}, lambda I: lib.gr_texture_decode(gr.handle, None, 145, scratch, 64, ref(I["output"])),
          byte_addressed=True)  # `out`, "output" in this entry point's messages
    plan = gr.fft_plan(capi.fft_options(16, 8, 1, 2, output_resource=capi.FFT_RESOURCE_TEXTURE))
    source = capi.fft_buffer_resource(buffer(16 * 8 * 8), 16 * 8 * 8, 16, 16 * 8)

    def fft(I):
        dst = capi.fft_image_resource(I["dst"])
        return lib.gr_fft_execute(gr.handle, None, plan, C.byref(dst), C.byref(source))
    entry("gr_fft_execute", {"dst": (*S, capi.FORMAT_R32G32_SFLOAT)}, fft, embedded=["dst"])
    gr.fft_plan_destroy(plan)
    print(json.dumps(out))


def run_worker(lib_dir=None):
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))  # in front of whatever is preloaded already
    if lib_dir:
        env["GRANITE_LIB_DIR"] = lib_dir
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# The fused bloom launches share their rules (post.hip: down_pair_fits), which call the three levels in, fine and coarse; gr_bloom_pyramid
# reports two images that share bytes as levels[i], levels[j].
SAYS = {("gr_bloom_down_mid", "threshold"): "in", ("gr_bloom_down_mid", "d0"): "fine", ("gr_bloom_down_mid", "d1"): "coarse",
        ("gr_bloom_down_tail", "d1"): "in", ("gr_bloom_down_tail", "d2"): "fine", ("gr_bloom_down_tail", "d3"): "coarse",
        ("gr_bloom_pyramid", "d2"): "fine", ("gr_bloom_pyramid", "d3"): "coarse"}


def names_the_argument(case, message):
    """gr_fxaa:T1 pitch+1:out -> `out` as a whole word in what follows "gr_fxaa_rows: invalid argument: " (every message holds "in" somewhere)"""
    function, what, argument = case.split(":")
    argument = argument.split("<")[0]
    said = argument if "row_into" in what else SAYS.get((function, argument), argument)  # images that share bytes go by the entry point's names
    if function == "gr_bloom_pyramid" and "row_into" in what:
        said = "levels"
    text = message.split(": ", 1)[-1].replace("invalid argument: ", "", 1)
    return re.search(rf"(?<![A-Za-z0-9_]){re.escape(said)}(?![A-Za-z0-9_])", text) is not None


def test_malformed_images_are_refused_and_the_rest_is_unchanged():
    got = run_worker()
    with open(PARENT) as f:
        parent = json.load(f)
    assert sorted(got) == sorted(parent)
    wrong = []
    for case, (code, message, launches) in sorted(got.items()):
        if code < 0 and launches != 0:
            wrong.append((case, "a refusal launched", code, launches))
        if case.split(":")[1].startswith("T"):
            if code != INVALID or launches != 0 or not names_the_argument(case, message):
                wrong.append((case, "a tightened case is not refused by name", code, message, launches))
        elif [code, launches] != parent[case]:
            wrong.append((case, "differs from the parent", [code, launches], parent[case], message))
    assert not wrong, wrong
    # the valid calls are there and launch: the table is not a list of refusals only
    valid = {case: row for case, row in got.items() if case.endswith(":valid")}
    assert len(valid) == 34 and all(code == 0 and launches >= 1 for code, _, launches in valid.values()), valid
    # gr_lighting's row band: {0, 0} is the whole target, {8, 1} lies below the last row
    assert got["gr_lighting:rows{0, 0}"] == [0, "", 1] and got["gr_lighting:rows{4, 2}"] == [0, "", 1] and got["gr_lighting:rows{6, 100}"] == [0, "", 1]
    assert got["gr_lighting:rows{8, 1}"] == [0, "", 0]
    assert got["gr_lighting:in_place:emissive=hdr"] == [0, "", 1]


if __name__ == "__main__":
    worker()
