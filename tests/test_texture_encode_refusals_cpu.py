"""CPU: what gr_texture_encode and gr_texture_generate_mipmap refuse, against the device-less HIP stand-in of tests/hip_stub: the
returned code, a message that names the argument or the rule, and no launch.  Valid calls launch once; an empty image returns GR_OK
without a launch.  These cases describe memory a kernel must not touch, so none of them may run on a device.

Run as a program (the worker of the test) it prints {case: [code, message, launches]}."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
INVALID, UNSUPPORTED = -1, -3


def worker():
    sys.path.insert(0, ROOT)
    from granite_amd import capi
    from granite_amd.capi import Image

    stub = C.CDLL(STUB)
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib = gr.lib
    R8, RG8, RGBA8, SRGB8 = capi.FORMAT_R8_UNORM, capi.FORMAT_R8G8_UNORM, capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8G8B8A8_SRGB
    BC4, BC5 = capi.FORMAT_BC4_UNORM_BLOCK, capi.FORMAT_BC5_UNORM_BLOCK
    keep = [capi.DeviceBuffer(gr, 1 << 17) for _ in range(3)]  # stay allocated for the run
    pixels, blocks, other = (b.ptr for b in keep)
    out = {}

    def counted(name, fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        out[name] = [code, lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    def image(w, h, fmt, pitch=None, ptr=pixels):
        return Image(ptr, w, h, w * capi.FORMAT_BPP[fmt] if pitch is None else pitch, fmt)

    def encode(name, fmt, img, dst=blocks, pitch=None):
        nbytes = 16 if fmt == BC5 else 8
        row = (img.width + 3) // 4 * nbytes if img is not None else 64
        counted("encode:" + name, lambda: lib.gr_texture_encode(gr.handle, None, fmt, C.byref(img) if img is not None else None, dst, row if pitch is None else pitch))

    encode("valid_bc4_r8", BC4, image(13, 6, R8))
    encode("valid_bc4_rg8", BC4, image(13, 6, RG8))
    encode("valid_bc4_srgb8", BC4, image(13, 6, SRGB8))
    encode("valid_bc5_rg8", BC5, image(13, 6, RG8))
    encode("valid_bc5_rgba8", BC5, image(13, 6, RGBA8))
    encode("valid_odd_pointer_and_pitch", BC5, image(13, 6, RG8, pitch=31, ptr=pixels + 3))
    encode("valid_wide_block_pitch", BC4, image(13, 6, R8), pitch=4 * 8 + 16)
    encode("valid_65536", BC4, image(65536, 1, R8))
    encode("empty_width", BC4, image(0, 6, R8))
    encode("empty_height", BC5, image(13, 0, RG8))
    encode("null_image", BC4, None)
    encode("block_format_bc7", 145, image(13, 6, RGBA8))
    encode("block_format_bc4_snorm", 140, image(13, 6, R8))
    encode("input_format", BC4, image(13, 6, capi.FORMAT_R16_SFLOAT))
    encode("bc5_from_r8", BC5, image(13, 6, R8))
    encode("width_above_65536", BC4, image(65537, 1, R8))
    encode("height_above_65536", BC4, image(1, 65537, R8))
    encode("pitch_short", BC5, image(13, 6, RG8, pitch=25))
    encode("null_pixels", BC4, image(13, 6, R8, ptr=None))
    encode("null_blocks", BC4, image(13, 6, R8), dst=None)
    encode("blocks_misaligned_bc4", BC4, image(13, 6, R8), dst=blocks + 4)
    encode("blocks_misaligned_bc5", BC5, image(13, 6, RG8), dst=blocks + 8)
    encode("block_pitch_misaligned", BC5, image(13, 6, RG8), pitch=4 * 16 + 8)
    encode("block_pitch_short", BC4, image(13, 6, R8), pitch=3 * 8)
    counted("encode:null_ctx", lambda: lib.gr_texture_encode(None, None, BC4, C.byref(image(13, 6, R8)), blocks, 32))

    def mip(name, src, dst):
        counted("mip:" + name, lambda: lib.gr_texture_generate_mipmap(gr.handle, None, C.byref(src) if src is not None else None,
                                                                       C.byref(dst) if dst is not None else None))

    for fmt, tag in ((R8, "r8"), (RG8, "rg8"), (RGBA8, "rgba8")):
        mip("valid_" + tag, image(13, 6, fmt), image(6, 3, fmt, ptr=other))
    mip("valid_1x9", image(1, 9, R8), image(1, 4, R8, ptr=other))
    mip("valid_odd_pointers", image(13, 6, RG8, pitch=29, ptr=pixels + 1), image(6, 3, RG8, pitch=15, ptr=other + 1))
    mip("srgb", image(13, 6, SRGB8), image(6, 3, SRGB8, ptr=other))
    mip("format", image(13, 6, capi.FORMAT_R16_SFLOAT), image(6, 3, capi.FORMAT_R16_SFLOAT, ptr=other))
    mip("formats_differ", image(13, 6, RG8), image(6, 3, R8, ptr=other))
    mip("null_src", None, image(6, 3, R8, ptr=other))
    mip("null_dst", image(13, 6, R8), None)
    mip("null_src_ptr", image(13, 6, R8, ptr=None), image(6, 3, R8, ptr=other))
    mip("null_dst_ptr", image(13, 6, R8), image(6, 3, R8, ptr=None))
    mip("empty_src", image(0, 6, R8), image(1, 3, R8, ptr=other))
    mip("src_above_65536", image(65537, 1, R8), image(32768, 1, R8, ptr=other))
    mip("dst_width", image(13, 6, R8), image(7, 3, R8, ptr=other))
    mip("dst_height", image(13, 6, R8), image(6, 2, R8, ptr=other))
    mip("dst_not_halved", image(13, 6, R8), image(13, 6, R8, ptr=other))
    mip("src_pitch_short", image(13, 6, RG8, pitch=25), image(6, 3, RG8, ptr=other))
    mip("dst_pitch_short", image(13, 6, RG8), image(6, 3, RG8, pitch=11, ptr=other))
    mip("shared_bytes", image(13, 6, R8), image(6, 3, R8, ptr=pixels + 13 * 5))
    counted("mip:null_ctx", lambda: lib.gr_texture_generate_mipmap(None, None, C.byref(image(13, 6, R8)), C.byref(image(6, 3, R8, ptr=other))))

    out["supported"] = [[b, i, lib.gr_texture_encode_supported(b, i)] for b in (BC4, BC5, 140, 145, R8) for i in (R8, RG8, RGBA8, SRGB8, capi.FORMAT_R16_SFLOAT, BC4)]
    print(json.dumps(out))


def run_worker():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))  # in front of whatever is preloaded already
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# case -> (code, words the message must hold)
REFUSALS = {
    "encode:null_image": (INVALID, ["in"]),
    "encode:block_format_bc7": (UNSUPPORTED, ["145", "block format"]),
    "encode:block_format_bc4_snorm": (UNSUPPORTED, ["140", "block format"]),
    "encode:input_format": (UNSUPPORTED, ["input format 76"]),
    "encode:bc5_from_r8": (UNSUPPORTED, ["input format 9", "one component"]),
    "encode:width_above_65536": (INVALID, ["65537", "65536"]),
    "encode:height_above_65536": (INVALID, ["65537", "65536"]),
    "encode:pitch_short": (INVALID, ["in pitch_bytes does not cover a row"]),
    "encode:null_pixels": (INVALID, ["in->ptr"]),
    "encode:null_blocks": (INVALID, ["blocks"]),
    "encode:blocks_misaligned_bc4": (INVALID, ["blocks", "multiple of the block size 8"]),
    "encode:blocks_misaligned_bc5": (INVALID, ["blocks", "multiple of the block size 16"]),
    "encode:block_pitch_misaligned": (INVALID, ["block_row_pitch_bytes (72)", "multiple of the block size 16"]),
    "encode:block_pitch_short": (INVALID, ["block row pitch 24", "4 blocks"]),
    "mip:srgb": (UNSUPPORTED, ["src_level", "R8G8B8A8_SRGB"]),
    "mip:format": (UNSUPPORTED, ["src_level format 76"]),
    "mip:formats_differ": (UNSUPPORTED, ["dst_level format 9", "src_level's format 16"]),
    "mip:null_src": (INVALID, ["src_level"]),
    "mip:null_dst": (INVALID, ["dst_level"]),
    "mip:null_src_ptr": (INVALID, ["src_level->ptr"]),
    "mip:null_dst_ptr": (INVALID, ["dst_level->ptr"]),
    "mip:empty_src": (INVALID, ["src_level has no texels"]),
    "mip:src_above_65536": (INVALID, ["src_level", "65537", "65536"]),
    "mip:dst_width": (INVALID, ["dst_level is 7 x 3", "6 x 3"]),
    "mip:dst_height": (INVALID, ["dst_level is 6 x 2", "6 x 3"]),
    "mip:dst_not_halved": (INVALID, ["dst_level is 13 x 6", "6 x 3"]),
    "mip:src_pitch_short": (INVALID, ["src_level pitch_bytes does not cover a row"]),
    "mip:dst_pitch_short": (INVALID, ["dst_level pitch_bytes does not cover a row"]),
    "mip:shared_bytes": (INVALID, ["dst_level shares bytes with src_level"]),
}


def test_refusals_name_their_reason_and_launch_nothing():
    got = run_worker()
    supported = got.pop("supported")
    wrong = []
    for case, (code, message, launches) in sorted(got.items()):
        if case in REFUSALS:
            want, words = REFUSALS[case]
            if code != want or launches != 0 or not all(w in message for w in words):
                wrong.append((case, code, message, launches))
        elif case.endswith("null_ctx"):
            if code != INVALID or launches != 0:
                wrong.append((case, code, launches))
        elif ":empty_" in case:
            if [code, launches] != [0, 0]:
                wrong.append((case, "an empty image returns GR_OK without a launch", code, message, launches))
        elif [code, launches] != [0, 1]:
            wrong.append((case, "a valid call launches once", code, message, launches))
    assert not wrong, wrong
    assert set(REFUSALS) <= set(got) and sum(":valid" in c for c in got) == 13
    for case, (code, message, _) in got.items():
        if case in REFUSALS:
            assert message.startswith("gr_texture_encode: " if case.startswith("encode") else "gr_texture_generate_mipmap: "), (case, message)
    takes = {(139, 9), (139, 16), (139, 37), (139, 43), (141, 16), (141, 37), (141, 43)}
    assert all(answer == (1 if (b, i) in takes else 0) for b, i, answer in supported), supported


if __name__ == "__main__":
    worker()
