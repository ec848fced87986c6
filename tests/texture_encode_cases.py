"""TEST INFRASTRUCTURE.  The cases of the texture encoder (gr_texture_encode, gr_texture_generate_mipmap), shared by the recording script
(tests/golden/make_texture_encode_golden.py), the CPU tests and the GPU tests.  The inputs are made here from a fixed seed and stored in
tests/golden/texture_encode_v1.npz beside what the reference's own code made of them; tests read them from there.

Encode cases: name -> (width, height, input format, block formats).  Mip cases: name -> (format, width, height, layers, levels)."""
import os

import numpy as np

SEED = 20261020
R8, RG8, RGBA8, SRGB8 = 9, 16, 37, 43
BC4, BC5 = 139, 141
CHANNELS = {R8: 1, RG8: 2, RGBA8: 4, SRGB8: 4}
BLOCK_BYTES = {BC4: 8, BC5: 16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_encode_v1.npz")

ENCODE_CASES = {
    "one": (1, 1, R8, (BC4,)),               # one texel clamp-padded into a flat block
    "edge_r8": (5, 7, R8, (BC4,)),           # partial blocks on both axes
    "edge_rg8": (13, 6, RG8, (BC5,)),        # two channels, partial blocks
    "edge_rgba8": (9, 9, SRGB8, (BC4, BC5)),  # stride 4; blue and alpha are noise that must not matter
    "hand": (24, 4, R8, (BC4,)),             # HAND_BLOCKS
    "tiles": (32, 32, R8, (BC4,)),           # every 4 x 4 block constant: 64 flat blocks
    "uniform": (128, 128, R8, (BC4,)),
    "gradient": (128, 128, R8, (BC4,)),
    "masks": (128, 128, R8, (BC4,)),
    "levels": (128, 128, R8, (BC4,)),
}
FAMILIES = ("uniform", "gradient", "masks", "levels")

# 16 texels row by row, then what the reference gave: endpoints and the 48 index bits.
HAND_BLOCKS = [
    ([0] * 7 + [255] * 8 + [128], (0, 128), 0x3fffffe00000),   # error 0 first at lo = 0, hi = 7; (128, 128) has error 0 too and must lose
    ([0, 255] * 4 + [255, 0] * 4, (255, 0), 0x208208041041),   # the 7-weight error is 0: nothing may replace it
    (list(range(100, 116)), (115, 100), 0x0126e4b76fc9),       # range 15: no search
    (list(range(100, 115)) + [116], (116, 100), 0x093724b76fc9),  # range 16: the threshold
    ([77] * 16, (77, 77), 0),                                  # flat
    ([0] * 4 + [10] * 4 + [20] * 4 + [255] * 4, (10, 20), 0xfff249000db6),  # both out-of-range codes, 6 and 7
]

MIP_CASES = {
    "r8_5x3": (R8, 5, 3, 1, 3),          # 5 -> 2 -> 1 and 3 -> 1 -> 1: weights that are no halves
    "rg8_16x16": (RG8, 16, 16, 1, 5),    # pure 2 : 1, weights exactly 0.5; filled for exact .5 values before rounding
    "rgba8_7x13": (RGBA8, 7, 13, 1, 4),
    "r8_1x9": (R8, 1, 9, 1, 4),          # the width stays 1
    "rgba8_6x6_layers": (RGBA8, 6, 6, 2, 3),
    "rg8_12x12_two": (RG8, 12, 12, 1, 2),  # 2 of its 4 levels
}
GTX_LEVELS = 4  # the full chain of the 13 x 6 edge_rg8 image: 13 x 6, 6 x 3, 3 x 1, 1 x 1


def blocks_to_image(blocks):
    """(by, bx, 16) texel blocks, row by row inside a block, to a (4 by, 4 bx) image."""
    by, bx, _ = blocks.shape
    return np.ascontiguousarray(blocks.reshape(by, bx, 4, 4).transpose(0, 2, 1, 3).reshape(4 * by, 4 * bx).astype(np.uint8))


def family_blocks(name, rng, by, bx):
    """(by, bx, 16) uint8 of one content family."""
    n = by * bx
    if name == "uniform":
        t = rng.integers(0, 256, (n, 16))
    elif name == "gradient":  # a base plus an x / y slope in +-16 plus noise of amplitude 0 - 5, clamped
        base, sx, sy = rng.integers(0, 256, (n, 1)), rng.integers(-16, 17, (n, 1)), rng.integers(-16, 17, (n, 1))
        amplitude = rng.integers(0, 6, (n, 1))
        x, y = np.arange(16)[None, :] % 4, np.arange(16)[None, :] // 4
        noise = np.rint(rng.uniform(-1.0, 1.0, (n, 16)) * amplitude).astype(np.int64)
        t = np.clip(base + sx * x + sy * y + noise, 0, 255)
    elif name == "masks":  # about a quarter 0, a quarter 255, the rest a cluster of width 1 - 40 around a mid value
        mid, width = rng.integers(40, 216, (n, 1)), rng.integers(1, 41, (n, 1))
        cluster = np.clip(mid + np.rint(rng.uniform(-0.5, 0.5, (n, 16)) * width).astype(np.int64), 0, 255)
        pick = rng.uniform(0.0, 1.0, (n, 16))
        t = np.where(pick < 0.25, 0, np.where(pick < 0.5, 255, cluster))
    elif name == "levels":  # 2 - 4 random levels a block
        values, count = rng.integers(0, 256, (n, 4)), rng.integers(2, 5, (n, 1))
        t = np.take_along_axis(values, rng.integers(0, 4, (n, 16)) % count, axis=1)
    else:
        raise KeyError(name)
    return t.astype(np.uint8).reshape(by, bx, 16)


def make_encode_inputs():
    """name -> (height, width, channels) uint8."""
    rng = np.random.default_rng(SEED)
    out = {}
    for name, (w, h, fmt, _) in ENCODE_CASES.items():
        if name == "hand":
            image = blocks_to_image(np.array([b[0] for b in HAND_BLOCKS], np.uint8).reshape(1, len(HAND_BLOCKS), 16))
        elif name == "tiles":
            image = blocks_to_image(np.repeat(rng.integers(0, 256, (h // 4, w // 4, 1)), 16, axis=2))
        elif name in FAMILIES:
            image = blocks_to_image(family_blocks(name, rng, h // 4, w // 4))
        else:
            image = rng.integers(0, 256, (h, w, CHANNELS[fmt]), dtype=np.uint8)
        out[name] = np.ascontiguousarray(image.reshape(h, w, CHANNELS[fmt]))
    return out


def make_mip_inputs():
    """name -> (layers, height, width, channels) uint8, level 0."""
    rng = np.random.default_rng(SEED + 1)
    out = {}
    for name, (fmt, w, h, layers, _) in MIP_CASES.items():
        image = rng.integers(0, 256, (layers, h, w, CHANNELS[fmt]), dtype=np.uint8)
        if name == "rg8_16x16":  # 2 x 2 quads (a, a, a + 1, a + 1) in some order: their mean is a + 0.5
            a = rng.integers(0, 255, (layers, h // 2, w // 2, CHANNELS[fmt]))
            quad = np.stack([a, a, a + 1, a + 1], axis=-1)
            quad = np.take_along_axis(quad, np.argsort(rng.uniform(size=quad.shape), axis=-1), axis=-1)  # (l, h/2, w/2, c, 4)
            image = quad.reshape(layers, h // 2, w // 2, CHANNELS[fmt], 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(layers, h, w, CHANNELS[fmt]).astype(np.uint8)
        out[name] = np.ascontiguousarray(image)
    return out


def level_extent(v, level):
    return max(v >> level, 1)


def chain_layout(fmt, w, h, layers, levels):
    """[(offset, width, height)] of a GTX payload's levels and its size: levels 16-byte aligned, layers inside a level."""
    out, offset = [], 0
    for l in range(levels):
        offset = (offset + 15) & ~15
        lw, lh = level_extent(w, l), level_extent(h, l)
        out.append((offset, lw, lh))
        offset += lw * lh * CHANNELS[fmt] * layers
    return out, offset


def chain_level(payload, fmt, w, h, layers, levels, level):
    """(layers, height, width, channels) view of one level of a chain payload."""
    layout, _ = chain_layout(fmt, w, h, layers, levels)
    offset, lw, lh = layout[level]
    c = CHANNELS[fmt]
    return payload[offset:offset + layers * lh * lw * c].reshape(layers, lh, lw, c)


def load_golden():
    return np.load(GOLDEN)
