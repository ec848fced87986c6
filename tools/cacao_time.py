"""The SSAO pass (FidelityFX CACAO, csrc/cacao.hip) on the synthetic G-buffer at 3840 x 2160 and 1920 x 1080, quality HIGHEST (what
setup_ffx_cacao installs: adaptive, 2 blur passes) and HIGH, chained entry point by entry point on one stream as Granite::setup_ffx_cacao
chains it (tests/test_gpu_cacao_pass.py holds the pass to this chain byte for byte).

Two measurements.  Wall clock the way tools/fft_time.py takes it: 2 warm-up calls, then 10 back-to-back calls between two
synchronisations, three rounds, every one printed -- beside a device copy (gr_copy) of the bytes the pass has to move, in the same run.
Then the split inside one pass by events: the library's own event brackets around every entry point (gr_timing_*), per stage over 10
passes.  The brackets serialise the launches, so the event split adds up to more than the wall clock.

Bytes the pass has to move, per full-resolution pixel (every intermediate written once and read once by the stage that consumes it; the
depth taps of the generate kernels, which re-read the R16F layers up to 64 times a texel through the caches, are counted once):
prepare depths 4 + 2.66, prepare normals 4 + 4, generate base 2 + 4 + 2, importance map 2, generate 2 + 4 + 2 + 2, blur 2 + 2,
apply 2 + 1 = 41.66 bytes at HIGHEST; without the base pass and the importance map 31.66 at HIGH.

    timeout -k 10 300 python tools/cacao_time.py > profiles/cacao_time.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fft_time import per_call_ms  # noqa: E402
from granite_amd import capi, synth  # noqa: E402

BYTES_PER_PIXEL = {capi.CACAO_QUALITY_HIGHEST: 4 + 8 / 3 + 8 + 8 + 2 + 10 + 4 + 3, capi.CACAO_QUALITY_HIGH: 4 + 8 / 3 + 8 + 10 + 4 + 3}
STAGES = ("cacao_prepare_depths", "cacao_prepare_normals", "cacao_generate_base", "cacao_importance_generate", "cacao_importance_postprocess_a",
          "cacao_importance_postprocess_b", "cacao_generate_q3", "cacao_generate_q2", "cacao_blur", "cacao_apply")


def main():
    gr = capi.Context(0)
    scratch_a, scratch_b = capi.DeviceBuffer(gr, 256 << 20), capi.DeviceBuffer(gr, 256 << 20)
    for w, h in ((3840, 2160), (1920, 1080)):
        cam = synth.Camera(w, h)
        g = synth.make_gbuffer(cam)
        depth = capi.DeviceImage(gr, w, h, capi.FORMAT_D32_SFLOAT).upload(g["depth"])
        normal = capi.DeviceImage(gr, w, h, capi.FORMAT_A2B10G10R10_UNORM_PACK32).upload(g["normal"])
        out = capi.DeviceImage(gr, w, h, capi.FORMAT_R8_UNORM)
        workspace = gr.cacao_workspace(w, h)
        rp = cam.render_params()
        for quality, name in ((capi.CACAO_QUALITY_HIGHEST, "HIGHEST"), (capi.CACAO_QUALITY_HIGH, "HIGH")):
            settings = capi.cacao_reference_settings()
            settings.quality_level = quality
            constants = capi.cacao_constants(w, h, rp[0:16], rp[16:32], settings, ctx=gr)

            def run():
                gr.cacao(depth, normal, out, workspace, constants, quality, settings.blur_pass_count)

            moved = int(BYTES_PER_PIXEL[quality] * w * h)
            for round_ in range(3):
                ms = per_call_ms(gr, run)
                copy_ms = per_call_ms(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, scratch_b.ptr, scratch_a.ptr, moved // 2)))
                print(f"{w} x {h} {name:7s} round {round_}: {ms * 1e3:8.1f} us;  {moved / 1e6:6.1f} MB moved;  copy of those bytes {copy_ms * 1e3:7.1f} us;"
                      f"  ratio {ms / copy_ms:5.2f}")
            gr.timing_enable(True)
            run()
            gr.sync()
            gr.timing_reset()
            for _ in range(10):
                run()
            gr.sync()
            q = gr.timing_query()
            total = 0.0
            for stage in STAGES:
                count, stage_ms = q.get(stage, (0, 0.0))[:2]
                if count:
                    total += stage_ms
                    print(f"{w} x {h} {name:7s} events: {stage:32s} {stage_ms * 100:8.1f} us a pass")
            print(f"{w} x {h} {name:7s} events: {'sum':32s} {total * 100:8.1f} us a pass")
            gr.timing_enable(False)
            mean = float(out.download().mean())
            print(f"{w} x {h} {name:7s} mean ambient occlusion {mean:.2f} of 255")
    gr.close()


if __name__ == "__main__":
    main()
