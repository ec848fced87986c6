"""TEST INFRASTRUCTURE.  The block sets the BC decode tests share: for every format the branches a decoder can take, forced into random
blocks (every BC7 mode and the reserved pattern, every value of BC6H's low five bits, BC1's equal and tie-sum endpoints, RGTC's equal and
ascending endpoints), and the mip-tail sizes where block counts round up.  cases() -> {name: (format, width, height, blocks)} generates
them (tests/golden/make_bc_decode_golden.py records them); golden() -> {name: (format, width, height, blocks, out)} reads them back with
what the reference's decode shaders, executed on the CPU, stored for them (tests/golden/bc_decode_shader_v1.npz)."""
import os

import numpy as np

import bc_ref

TAIL_SIZES = ((1, 1), (2, 2), (5, 3), (13, 7))


def _random(rng, count, nbytes):
    return rng.integers(0, 256, (count, nbytes), dtype=np.uint8)


def _grid(blocks, per_row):
    """(format-agnostic) blocks laid out per_row to a row -> (width, height, blocks)."""
    rows = len(blocks) // per_row
    assert rows * per_row == len(blocks)
    return 4 * per_row, 4 * rows, blocks.reshape(rows, per_row, -1)


def _set_u16(blocks, at, values):
    blocks[:, at] = values & 0xff
    blocks[:, at + 1] = values >> 8


def cases():
    rng = np.random.default_rng(20261017)
    out = {}
    # BC7: 9 x 32 blocks, mode bits forced (mode m = bit m the lowest set; the ninth group has a zero low byte)
    b = _random(rng, 288, 16)
    for i in range(288):
        m = i // 32
        b[i, 0] = 0 if m == 8 else ((int(b[i, 0]) >> (m + 1)) << (m + 1) | (1 << m)) & 0xff
    out["bc7_modes"] = (bc_ref.BC7_UNORM,) + _grid(b, 18)
    out["bc7_13x7"] = (bc_ref.BC7_UNORM, 13, 7, _random(rng, 8, 16).reshape(2, 4, 16))
    # BC6H: 32 x 16 blocks, the low five bits forced
    for name, fmt in (("bc6h_ufloat", bc_ref.BC6H_UFLOAT), ("bc6h_sfloat", bc_ref.BC6H_SFLOAT)):
        b = _random(rng, 512, 16)
        b[:, 0] = (b[:, 0] & 0xe0) | (np.arange(512) // 16).astype(np.uint8)
        out[name + "_modes"] = (fmt,) + _grid(b, 16)
        out[name + "_13x7"] = (fmt, 13, 7, _random(rng, 8, 16).reshape(2, 4, 16))
    # BC1: random, equal endpoints, three-colour blocks whose endpoint sums are the tie sums (31 in a 5-bit channel; 21, 63, 105 in green)
    for name, fmt in (("bc1_rgb", bc_ref.BC1_RGB_UNORM), ("bc1_rgba", bc_ref.BC1_RGBA_UNORM)):
        out[name + "_random"] = (fmt,) + _grid(_random(rng, 256, 8), 16)
        b = _random(rng, 64, 8)
        b[:, 2:4] = b[:, 0:2]
        out[name + "_equal"] = (fmt,) + _grid(b, 8)
        b = _random(rng, 64, 8)
        r0, g0, b0 = rng.integers(0, 32, 64), rng.integers(0, 64, 64), rng.integers(0, 32, 64)
        r1, b1 = 31 - r0, 31 - b0
        g_sum = rng.choice([21, 63, 105], 64)
        g0 = np.clip(g0, np.maximum(g_sum - 63, 0), np.minimum(g_sum, 63))
        g1 = g_sum - g0
        c0, c1 = (r0 << 11) | (g0 << 5) | b0, (r1 << 11) | (g1 << 5) | b1
        lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)  # color0 <= color1: the three-colour mode
        _set_u16(b, 0, lo.astype(np.uint16))
        _set_u16(b, 2, hi.astype(np.uint16))
        out[name + "_tie_sums"] = (fmt,) + _grid(b, 8)
    out["bc2_random"] = (bc_ref.BC2_UNORM,) + _grid(_random(rng, 128, 16), 16)
    out["bc3_random"] = (bc_ref.BC3_UNORM,) + _grid(_random(rng, 128, 16), 16)
    for name, fmt, nbytes in (("bc4", bc_ref.BC4_UNORM, 8), ("bc5", bc_ref.BC5_UNORM, 16)):
        out[name + "_random"] = (fmt,) + _grid(_random(rng, 128, nbytes), 16)
        b = _random(rng, 32, nbytes)
        b[:, 1::8] = b[:, 0::8]
        out[name + "_equal"] = (fmt,) + _grid(b, 8)
        b = _random(rng, 32, nbytes)
        for at in range(0, nbytes, 8):
            e = np.sort(b[:, at:at + 2], axis=1)
            e[:, 1] = np.maximum(e[:, 1], e[:, 0].astype(int) + 1).clip(0, 255)
            e[:, 0] = np.minimum(e[:, 0], e[:, 1].astype(int) - 1).clip(0, 255)
            b[:, at:at + 2] = e
        out[name + "_ascending"] = (fmt,) + _grid(b, 8)
    for w, h in TAIL_SIZES:
        bw, bh = (w + 3) // 4, (h + 3) // 4
        out[f"bc1_tail_{w}x{h}"] = (bc_ref.BC1_RGBA_UNORM, w, h, _random(rng, bw * bh, 8).reshape(bh, bw, 8))
        out[f"bc3_tail_{w}x{h}"] = (bc_ref.BC3_UNORM, w, h, _random(rng, bw * bh, 16).reshape(bh, bw, 16))
    return out


_GOLDEN = {}
_REFERENCE = {}


def golden():
    if not _GOLDEN:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc_decode_shader_v1.npz")) as z:
            for name in sorted({k.split("/")[0] for k in z.files}):
                fmt, w, h = (int(v) for v in z[name + "/format"])
                _GOLDEN[name] = (fmt, w, h, z[name + "/blocks"], z[name + "/out"])
    return _GOLDEN


def reference(name):
    """bc_ref's (image, ties) of a golden case, computed once."""
    if name not in _REFERENCE:
        fmt, w, h, blocks, _ = golden()[name]
        _REFERENCE[name] = bc_ref.decode(fmt, blocks, w, h)
    return _REFERENCE[name]
