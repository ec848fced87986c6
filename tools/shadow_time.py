"""Directional shadows (csrc/shadow.hip) at 3840 x 2160 with 4096 positional lights and 2048 x 2048 x 4 shadow maps: what the separate
shadowed quad costs over the fused lighting kernel.  Device-event times from the library's own brackets around each entry point
(gr_timing_*): 5 warm-up calls, then 50 calls, three rounds, every one printed.

    fused        step (a): gr_lighting with the directional and the clustered bit, the unshadowed path
    pcf | wide | vsm
                 step (b): gr_directional_light in that mode (cascaded; D16 maps, R32G32F moments for vsm) followed by
                 gr_lighting(CLUSTERED) in place.  (b) - (a) is the cost of shadows in that mode.  Beside gr_directional_light's time stands
                 the rate at which it moves the 30 bytes a pixel of the frame's attachments (22 read, 8 written; shadow-map taps not counted).
    chain        step (c): gr_vsm_moments, the down blur and the up blur, one 2048 x 2048 layer (x 4 for the map)

Each step is a process of its own, so that each runs under its own time limit and nothing starts after a failure:

    for s in fused pcf wide vsm chain; do timeout -k 10 300 python tools/shadow_time.py $s || break; done > profiles/shadow_time.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from granite_amd import capi  # noqa: E402

W, H, LIGHTS, MAP = 3840, 2160, 4096, 2048
WARMUP, CALLS, ROUNDS = 5, 50, 3
FRAME_BYTES = W * H * 30


def rounds(gr, names, run):
    """-> per round {name: microseconds per call}"""
    out = []
    for _ in range(WARMUP):
        run()
    gr.sync()
    for _ in range(ROUNDS):
        gr.timing_reset()
        for _ in range(CALLS):
            run()
        gr.sync()
        got = gr.timing_query()
        for name in names:
            assert got[name][0] == CALLS, (name, got.get(name))
        out.append({name: got[name][1] * 1e3 / CALLS for name in names})
    return out


def transforms():
    out = np.zeros((4, 4, 4), np.float32)
    for i in range(4):
        r = 12.0 * 2.0 ** i
        out[i] = np.float32([[0.5 / r, 0, 0, 0.5], [0, 0, 0.5 / r, 0.5], [0, 1.0 / 128.0, 0, 0.5], [0, 0, 0, 1]])
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(4, 16)


def occluders(rng):
    blocks = rng.choice([0.35, 0.5, 0.5, 0.62], (MAP // 16, MAP // 16))
    return np.repeat(np.repeat(blocks, 16, 0), 16, 1) + rng.normal(0.0, 0.01, (MAP, MAP))


def lighting_steps(gr, step):
    import ctypes as C
    from gpu_scene import Scene
    scene = Scene(W, H, LIGHTS)
    built = scene.build_clusters_gpu(gr)
    both = capi.LIGHTING_DIRECTIONAL_BIT | capi.LIGHTING_CLUSTERED_BIT | capi.LIGHTING_AMBIENT_FALLBACK_BIT
    lighting, imgs = scene.lighting_args(gr, built, both if step == "fused" else capi.LIGHTING_CLUSTERED_BIT)
    if step == "fused":
        for i, r in enumerate(rounds(gr, ["lighting"], lambda: gr.check(gr.lib.gr_lighting(gr.handle, None, lighting)))):
            print(f"(a) fused gr_lighting, directional + clustered, {LIGHTS} lights: round {i}: {r['lighting']:8.1f} us")
        return
    rng = np.random.default_rng(3)
    a = capi.DirectionalLightArgs()
    a.albedo, a.normal, a.pbr, a.depth, a.emissive, a.hdr = lighting.albedo, lighting.normal, lighting.pbr, lighting.depth, lighting.hdr, lighting.hdr
    a.inv_view_projection[:] = list(lighting.inv_view_projection)
    C.memmove(C.byref(a.directional), C.byref(lighting.directional), C.sizeof(capi.PushDirectional))
    a.directional.cascade_log_bias = float(1.0 - np.log2(10.0))
    a.flags = capi.LIGHTING_AMBIENT_FALLBACK_BIT
    a.mode = {"pcf": capi.SHADOW_PCF, "wide": capi.SHADOW_PCF_WIDE, "vsm": capi.SHADOW_VSM}[step]
    a.layers = 4
    keep = []
    for i in range(4):
        field = occluders(rng)
        if step == "vsm":
            mx = field.astype(np.float32)
            layer = capi.DeviceImage(gr, MAP, MAP, capi.FORMAT_R32G32_SFLOAT).upload(np.stack([mx, mx * mx + np.float32(1e-3)], -1))
        else:
            layer = capi.DeviceImage(gr, MAP, MAP, capi.FORMAT_D16_UNORM).upload(np.rint(np.clip(field, 0, 1) * 65535.0).astype(np.uint16))
        keep.append(layer)
        a.shadow_maps[i] = layer.desc
    flat = transforms()
    for i in range(4):
        a.transforms[i][:] = [float(v) for v in flat[i]]

    def run():
        gr.directional_light(a)
        gr.check(gr.lib.gr_lighting(gr.handle, None, lighting))

    for i, r in enumerate(rounds(gr, ["directional_light", "lighting"], run)):
        d, l = r["directional_light"], r["lighting"]
        print(f"(b) {step:4s}: round {i}: gr_directional_light {d:8.1f} us ({FRAME_BYTES / d / 1e6:5.2f} TB/s of frame attachments) + gr_lighting(CLUSTERED) {l:8.1f} us = {d + l:8.1f} us")


def chain_step(gr):
    rng = np.random.default_rng(3)
    depth = capi.DeviceImage(gr, MAP, MAP, capi.FORMAT_D16_UNORM).upload(np.rint(np.clip(occluders(rng), 0, 1) * 65535.0).astype(np.uint16))
    raw, half, out = (capi.DeviceImage(gr, n, n, capi.FORMAT_R32G32_SFLOAT) for n in (MAP, MAP // 2, MAP))

    def run():
        gr.vsm_moments(depth, raw)
        gr.vsm_blur(raw, half, False)
        gr.vsm_blur(half, out, True)

    for i, r in enumerate(rounds(gr, ["vsm_moments", "vsm_down_blur", "vsm_up_blur"], run)):
        total = sum(r.values())
        print(f"(c) VSM chain, one {MAP} x {MAP} D16 layer: round {i}: moments {r['vsm_moments']:7.1f} us, down {r['vsm_down_blur']:7.1f} us, up {r['vsm_up_blur']:7.1f} us = "
              f"{total:7.1f} us a layer, {4 * total:7.1f} us the map")


def main():
    step = sys.argv[1] if len(sys.argv) > 1 else ""
    if step not in ("fused", "pcf", "wide", "vsm", "chain"):
        sys.exit(__doc__)
    gr = capi.Context(0)
    gr.timing_enable(True)
    if step == "chain":
        chain_step(gr)
    else:
        lighting_steps(gr, step)
    gr.timing_enable(False)
    gr.close()


if __name__ == "__main__":
    main()
