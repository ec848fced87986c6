"""Generates tests/golden/bloom_supported.json: the 0 / 1 answers of the five gr_bloom_*_supported queries over a sweep of frames.

The queries take no context and touch no device, so the kernel library answers them on any machine.  The committed table was written
with the library of the commit BEFORE the launch rules of post.hip were gathered into shared predicates; tests/test_bloom_supported_cpu.py
holds every later library to it.  Do not regenerate it to make that test pass: a changed answer is a changed launch.

cases() and answers() are what the test imports; running this file writes the table."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from granite_amd import capi  # noqa: E402
from oracle.oracle import level_size  # noqa: E402

FUNCTIONS = ("down_mid", "down_head", "tail", "up_all", "pyramid")
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bloom_supported.json")
LEVELS = (("threshold", 0.5), ("d0", 0.25), ("u0", 0.25), ("d1", 0.125), ("u1", 0.125), ("d2", 0.0625), ("u2", 0.0625), ("d3", 0.03125))
NAMES = ("hdr",) + tuple(name for name, _ in LEVELS) + ("history",)

BASELINE_CONFIGS = [(256, 256), (1920, 1080), (3840, 2160), (3840, 2160), (7680, 4320)]
# every frame size tests/test_gpu_post.py runs
GPU_POST_SIZES = [(256, 256), (250, 130), (70, 40), (64, 64), (1920, 1080), (33, 17), (128, 64), (16, 16), (3840, 2160), (7680, 4320), (2048, 2048),
                  (2560, 1440), (1280, 720), (1000, 808), (333, 250), (68, 90), (70, 38), (180, 256), (808, 333), (64, 48), (328, 200), (640, 360),
                  (200, 136), (72, 40), (330, 202), (1004, 812), (1002, 810), (101, 57), (80, 40), (40, 20), (18, 15), (13, 13)]
# Around each size limit, odd and even: 65536 texels of downsample-1 (a 2048 x 2048 frame), 960 x 540 of upsample-0 (3840 x 2160),
# 640 x 384 of the frame.  Multiples of 8 are where the head launch (every level exactly half) is possible at all.
OFFSETS = (-16, -8, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 8, 16)
LIMIT_GRID = [(cw + dx, ch + dy) for cw, ch in ((2048, 2048), (3840, 2160), (640, 384)) for dx in OFFSETS for dy in OFFSETS]
# what is done to a frame's descriptors before asking; on a few sizes, of which (640, 384) / (256, 256) / (1920, 1080) get "1"s unvaried
VARIANT_SIZES = [(256, 256), (640, 384), (1920, 1080), (250, 130), (2048, 2048)]
VARIANTS = ("hdr_ptr_plus_8", "hdr_pitch_plus_8", "threshold_ptr_plus_8", "d0_pitch_plus_8", "d0_is_d1", "history_is_d3", "u0_is_u1", "no_history",
            "d0_wider", "d1_taller", "d2_floor_half", "d3_floor_half", "u1_wider", "u1_narrower", "u2_not_d2", "history_smaller", "d3_one_row",
            "threshold_odd", "u0_odd")


def frame(w, h, b10):
    """The Image descriptors of a frame's bloom pass: fake device pointers (never dereferenced), 16-byte aligned and distinct, tight pitch."""
    sizes = {"hdr": (w, h)}
    sizes.update({name: level_size(w, h, scale) for name, scale in LEVELS})
    sizes["history"] = sizes["d3"]
    images = {}
    for i, name in enumerate(NAMES):
        fmt = capi.FORMAT_B10G11R11_UFLOAT_PACK32 if (b10 and name == "hdr") else capi.FORMAT_R16G16B16A16_SFLOAT
        iw, ih = sizes[name]
        images[name] = capi.Image(0x100000000 + i * 0x40000000, iw, ih, iw * capi.FORMAT_BPP[fmt], fmt)
    return images


def vary(im, variant):
    def resize(name, dw, dh):
        bpp = im[name].pitch_bytes // im[name].width
        im[name].width += dw
        im[name].height += dh
        im[name].pitch_bytes = im[name].width * bpp
    if variant == "hdr_ptr_plus_8":
        im["hdr"].ptr += 8
    elif variant == "hdr_pitch_plus_8":
        im["hdr"].pitch_bytes += 8
    elif variant == "threshold_ptr_plus_8":
        im["threshold"].ptr += 8
    elif variant == "d0_pitch_plus_8":
        im["d0"].pitch_bytes += 8
    elif variant == "d0_is_d1":
        im["d0"].ptr = im["d1"].ptr
    elif variant == "history_is_d3":
        im["history"].ptr = im["d3"].ptr
    elif variant == "u0_is_u1":
        im["u0"].ptr = im["u1"].ptr
    elif variant == "no_history":
        im["history"].ptr = None
    elif variant == "d0_wider":
        resize("d0", 1, 0)
    elif variant == "d1_taller":
        resize("d1", 0, 1)
    elif variant == "d2_floor_half":  # a level that is not ceil(half) of the one above where that one is odd, and a smaller one where it is even
        resize("d2", -1, -1)
    elif variant == "d3_floor_half":
        resize("d3", -1, -1)
    elif variant == "u1_wider":
        resize("u1", 2, 0)
    elif variant == "u1_narrower":
        resize("u1", -2, -2)
    elif variant == "u2_not_d2":
        resize("u2", 1, 0)
    elif variant == "history_smaller":
        resize("history", -1, 0)
    elif variant == "d3_one_row":  # the luminance reduction's size (downsample-3 / 2) comes out zero
        resize("d3", 0, 1 - im["d3"].height)
        resize("history", 0, 1 - im["history"].height)
    elif variant == "threshold_odd":
        resize("threshold", 1, 1)
    elif variant == "u0_odd":
        resize("u0", 1, 1)
    else:
        raise ValueError(variant)


def cases():
    """(id, images, with_luminance), ids unique and stable."""
    seen = set()
    for w, h in BASELINE_CONFIGS + GPU_POST_SIZES + LIMIT_GRID:
        if (w, h) in seen:
            continue
        seen.add((w, h))
        for b10 in (False, True):
            for lum in (False, True):
                yield "%dx%d %s %s" % (w, h, "b10" if b10 else "f16", "lum" if lum else "nolum"), frame(w, h, b10), lum
    for w, h in VARIANT_SIZES:
        for variant in VARIANTS:
            for b10 in (False, True):
                for lum in (False, True):
                    images = frame(w, h, b10)
                    vary(images, variant)
                    yield "%dx%d %s %s %s" % (w, h, "b10" if b10 else "f16", "lum" if lum else "nolum", variant), images, lum


def answers(lib, im, lum):
    """The five answers for one frame as a string of 0 / 1 in the order of FUNCTIONS, the push blocks built as the frame loop builds them."""
    down, up = capi.downsample_push, capi.upsample_push
    p_t = capi.threshold_push(im["threshold"])
    p_d0, p_d1 = down(im["d0"], im["threshold"]), down(im["d1"], im["d0"])
    p_d2, p_d3 = down(im["d2"], im["d1"], 0.25), down(im["d3"], im["d2"], 0.25)
    p_u2, p_u1, p_u0 = up(im["u2"], im["d3"]), up(im["u1"], im["u2"]), up(im["u0"], im["u1"])
    levels = {name: im[name] for name, _ in LEVELS}
    args = capi.pyramid_args(im["hdr"], levels, im["history"], 0.25, 0x7000000000 if lum else None, 0.5)
    out = (lib.gr_bloom_down_mid_supported(im["threshold"], im["d0"], im["d1"], p_d0, p_d1),
           lib.gr_bloom_down_head_supported(im["hdr"], im["threshold"], im["d0"], im["d1"], p_t, p_d0, p_d1),
           lib.gr_bloom_tail_supported(im["d1"], im["d2"], im["d3"], im["u2"], im["u1"], p_d2, p_d3, p_u2, p_u1),
           lib.gr_bloom_up_all_supported(im["d3"], im["u2"], im["u1"], im["u0"], p_u2, p_u1, p_u0),
           lib.gr_bloom_pyramid_supported(args))
    assert all(v in (0, 1) for v in out), out
    return "".join(str(v) for v in out)


if __name__ == "__main__":
    lib = capi.load_library()
    table = {name: answers(lib, images, lum) for name, images, lum in cases()}
    json.dump({"functions": FUNCTIONS, "answers": table}, open(PATH, "w"), indent=0, sort_keys=True)
    print("wrote", PATH, len(table), "cases")
