"""Records tests/golden/cacao_constants_v1.npz: FFX_CACAO_BufferSizeInfo and the four FFX_CACAO_Constants blocks as the reference's own
renderer/post/ffx-cacao/src/ffx_cacao.cpp computes them, for the test sizes, the two cameras, the two settings and both quality levels of
tests/cacao_cases.py.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  ffx_cacao.cpp is compiled from where it lies
with the runner next to this file into a temporary directory, run, and the directory is removed: the file holds data only.

    python tests/golden/make_cacao_golden.py [output.npz]

While recording it also runs tests/cacao_ref.py's float32 chain on every case and prints the share of texels it flags (a tap's lod within
2^-10 of a mip switch): the tests ask for at most 0.5 % in every case, so the scenes are chosen here, not there.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle", "ref_build")]
import cacao_cases as cc  # noqa: E402
import cacao_ref as cr  # noqa: E402
import shader_runner as sr  # noqa: E402

CACAO = os.path.join(sr.REF, "renderer", "post", "ffx-cacao")

FLAG_SHARE_LIMIT = 0.005


def build(tmp):
    objs = sr.compile_objects(tmp, ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-I" + os.path.join(CACAO, "inc")],
                              [("ffx_cacao", os.path.join(CACAO, "src", "ffx_cacao.cpp"), []), ("runner", os.path.join(HERE, "cacao_constants_runner.cpp"), [])])
    return sr.link(os.path.join(tmp, "libcacao_runner.so"), objs)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def generate(path):
    if not os.path.isdir(CACAO):
        raise FileNotFoundError(CACAO)
    record = {}
    with sr.scratch("cacao_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        assert [lib.cacao_runner_sizes(i) for i in range(3)] == [68, 384, 64]
        for w, h in cc.SIZES:
            for cam_name in cc.CAMERAS:
                proj, view = cc.matrices(cc.camera(cam_name, w, h))
                for variant in cc.SETTINGS:
                    for quality in cc.QUALITIES:
                        words = cc.settings_words(variant, quality)
                        sizes, constants = np.zeros(16, np.uint32), np.zeros(4 * 384, np.uint8)
                        lib.cacao_runner_constants(w, h, ptr(words), ptr(proj), ptr(view), ptr(sizes), ptr(constants))
                        k = cc.key(w, h, cam_name, variant, quality)
                        record[k + "/settings"], record[k + "/constants"] = words, constants
                        record[k + "/proj"], record[k + "/view"] = proj, view
                        record[f"{w}x{h}/sizes"] = sizes
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(record)} arrays")

    cc._golden = None
    worst = 0.0
    for case in cc.CASES:
        w, h, cam_name, variant, _ = case
        depth, normal = cc.case_inputs(case)
        for quality in cc.QUALITIES:
            r = cr.chain(depth, normal, cc.constants(w, h, cam_name, variant, quality), quality, 2)
            share = float(r["info"]["flag"].mean())
            if quality == cr.QUALITY_HIGHEST:
                share = max(share, float(r["base_info"]["flag"].mean()))
            worst = max(worst, share)
            print(f"{cc.case_id(case):40s} q{quality}: flagged {100 * share:.3f} %, taps {r['info']['taps'].min()} .. {r['info']['taps'].max()}, "
                  f"highest mip {r['info']['max_mip']}, a tap outside: {r['info']['outside']}, counter {r['load_counter']}")
    print(f"largest flagged share {100 * worst:.3f} % (limit {100 * FLAG_SHARE_LIMIT} %)")
    assert worst <= FLAG_SHARE_LIMIT


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else cc.GOLDEN_PATH)
