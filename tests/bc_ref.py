"""TEST INFRASTRUCTURE.  A plain Python decoder of BC1-BC7 blocks written from the formats' specification (Khronos Data Format
Specification, chapters S3TC, RGTC and BPTC), block by block, with no regard for speed.  It is the yardstick the device decode is
held to on sizes the golden of the executed shaders (tests/golden/bc_decode_shader_v1.npz) does not hold, and is itself held to that
golden, case by case, by tests/test_bc_ref_cpu.py.

BC1-BC5 samples are rationals (endpoints c * 255 / 31 and c * 255 / 63, interpolants at 1/3, 2/3 and 1/2, BC2 alpha a * 17, RGTC
(e0 * (d - k) + e1 * k) / d with d = 7 or 5); this decoder rounds the exact value to nearest and reports the samples whose exact value
ends in exactly 1/2 as *ties*: there either neighbour is a correct rounding (a float evaluation lands on one by chance).  BC6H and
BC7 are integer formats and have no ties."""
import numpy as np

BC1_RGB_UNORM, BC1_RGB_SRGB, BC1_RGBA_UNORM, BC1_RGBA_SRGB = 131, 132, 133, 134
BC2_UNORM, BC2_SRGB, BC3_UNORM, BC3_SRGB = 135, 136, 137, 138
BC4_UNORM, BC5_UNORM = 139, 141
BC6H_UFLOAT, BC6H_SFLOAT, BC7_UNORM, BC7_SRGB = 143, 144, 145, 146

BLOCK_BYTES = {131: 8, 132: 8, 133: 8, 134: 8, 135: 16, 136: 16, 137: 16, 138: 16, 139: 8, 141: 16, 143: 16, 144: 16, 145: 16, 146: 16}
# (channels, dtype) of the decoded image
DECODED = {139: (1, np.uint8), 141: (2, np.uint8), 143: (4, np.uint16), 144: (4, np.uint16)}


def _round(num, den):
    """num / den to nearest (halves up) and whether it was a half."""
    return (2 * num + den) // (2 * den), (2 * num) % (2 * den) == den


# ---- S3TC ------------------------------------------------------------------------------------------------------------------------

def _bc1_colours(block, always_four, punch_alpha):
    """16 x ((r, g, b, a), (tie r, tie g, tie b, tie a)) of the 8-byte colour block."""
    c0, c1 = block & 0xffff, (block >> 16) & 0xffff
    chan = lambda c: ((c >> 11, 31), ((c >> 5) & 63, 63), (c & 31, 31))
    pal = []
    e0, e1 = chan(c0), chan(c1)
    four = always_four or c0 > c1
    for k in range(4):
        texel, tie = [], []
        for (a, m), (b, _) in zip(e0, e1):
            if k == 0:
                v, t = _round(255 * a, m)
            elif k == 1:
                v, t = _round(255 * b, m)
            elif four:
                v, t = _round(255 * ((2 * a + b) if k == 2 else (a + 2 * b)), 3 * m)
            elif k == 2:
                v, t = _round(255 * (a + b), 2 * m)
            else:
                v, t = 0, False
            texel.append(v)
            tie.append(t)
        alpha = punch_alpha if (not four and k == 3) else 255
        pal.append((texel + [alpha], tie + [False]))
    return [pal[(block >> (32 + 2 * i)) & 3] for i in range(16)]


def _rgtc(block):
    """16 x (value, tie) of an 8-byte RGTC block."""
    e0, e1 = block & 0xff, (block >> 8) & 0xff
    out = []
    for i in range(16):
        k = (block >> (16 + 3 * i)) & 7
        if k == 0:
            out.append((e0, False))
        elif k == 1:
            out.append((e1, False))
        elif e0 > e1:
            out.append(_round(e0 * (7 - (k - 1)) + e1 * (k - 1), 7))
        elif k >= 6:
            out.append((0 if k == 6 else 255, False))
        else:
            out.append(_round(e0 * (5 - (k - 1)) + e1 * (k - 1), 5))
    return out


# ---- BPTC ------------------------------------------------------------------------------------------------------------------------

def _rows(text):
    return [[int(ch) for ch in row.replace(" ", "")] for row in text.strip().splitlines()]


# Partition sets for two subsets (64 shapes, texel 0 first) and three subsets, and the anchor (fix-up) indices, as the specification
# tabulates them.
_P2 = _rows("""
0011001100110011 0001000100010001 0111011101110111 0001001100110111 0000000100010011 0011011101111111 0001001101111111 0000000100110111
0000000000010011 0011011111111111 0000000101111111 0000000000010111 0001011111111111 0000000011111111 0000111111111111 0000000000001111
0000100011101111 0111000100000000 0000000010001110 0111001100010000 0011000100000000 0000100011001110 0000000010001100 0111001100110001
0011000100010000 0000100010001100 0110011001100110 0011011001101100 0001011111101000 0000111111110000 0111000110001110 0011100110011100
0101010101010101 0000111100001111 0101101001011010 0011001111001100 0011110000111100 0101010110101010 0110100101101001 0101101010100101
0111001111001110 0001001111001000 0011001001001100 0011101111011100 0110100110010110 0011110011000011 0110011010011001 0000011001100000
0100111001000000 0010011100100000 0000001001110010 0000010011100100 0110110010010011 0011011011001001 0110001110011100 0011100111000110
0110110011001001 0110001100111001 0111111010000001 0001100011100111 0000111100110011 0011001111110000 0010001011101110 0100010001110111
""".replace(" ", "\n"))
_P3 = _rows("""
0011001102212222 0001001122112221 0000200122112211 0222002200110111 0000000011221122 0011001100220022 0022002211111111 0011001122112211
0000000011112222 0000111111112222 0000111122222222 0012001200120012 0112011201120112 0122012201220122 0011011211221222 0011200122002220
0001001101121122 0111001120012200 0000112211221122 0022002200221111 0111011102220222 0001000122212221 0000001101220122 0000110022102210
0122012200110000 0012001211222222 0110122112210110 0000011012211221 0022110211020022 0110011020022222 0011012201220011 0000200022112221
0000000211221222 0222002200120011 0011001200220222 0120012001200120 0000111122220000 0120120120120120 0120201212010120 0011220011220011
0011112222000011 0101010122222222 0000000021212121 0022112200221122 0022001100220011 0220122102201221 0101222222220101 0000212121212121
0101010101012222 0222011102220111 0002111200021112 0000211221122112 0222011101110222 0002111211120002 0110011001102222 0000000021122112
0110011022222222 0022001100110022 0022112211220022 0000000000002112 0002000100020001 0222122202221222 0101222222222222 0111201122012220
""".replace(" ", "\n"))
_A2 = [15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
       15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15]
_A3_SECOND = [3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
              8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3]
_A3_THIRD = [15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
             15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8]
_WEIGHTS = {2: [0, 21, 43, 64], 3: [0, 9, 18, 27, 37, 46, 55, 64], 4: [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64]}


class _Reader:
    def __init__(self, block):
        self.block, self.at = block, 0

    def take(self, n):
        v = (self.block >> self.at) & ((1 << n) - 1)
        self.at += n
        return v


def _indices(reader, bits, anchors):
    out = []
    for i in range(16):
        out.append(reader.take(bits - 1 if i in anchors else bits))
    return out


# subsets, partition bits, rotation bits, index selection bits, colour bits, alpha bits, endpoint p-bits, shared p-bits, index bits, second index bits
_BC7_MODES = [(3, 4, 0, 0, 4, 0, 1, 0, 3, 0), (2, 6, 0, 0, 6, 0, 0, 1, 3, 0), (3, 6, 0, 0, 5, 0, 0, 0, 2, 0), (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
              (1, 0, 2, 1, 5, 6, 0, 0, 2, 3), (1, 0, 2, 0, 7, 8, 0, 0, 2, 2), (1, 0, 0, 0, 7, 7, 1, 0, 4, 0), (2, 6, 0, 0, 5, 5, 1, 0, 2, 0)]


def _bc7(block):
    """16 x (r, g, b, a)."""
    mode = 0
    while mode < 8 and not (block >> mode) & 1:
        mode += 1
    if mode == 8:
        return [(0, 0, 0, 0)] * 16  # reserved
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = _BC7_MODES[mode]
    rd = _Reader(block)
    rd.take(mode + 1)
    shape, rotation, index_selection = rd.take(pb), rd.take(rb), rd.take(isb)
    ends = [[[0, 0, 0, 255] for _ in range(2)] for _ in range(ns)]
    for c in range(4 if ab else 3):
        for s in range(ns):
            for e in range(2):
                ends[s][e][c] = rd.take(cb if c < 3 else ab)
    precision = [cb, cb, cb, ab]
    if epb or spb:
        for s in range(ns):
            shared = rd.take(1) if spb else None
            for e in range(2):
                p = shared if spb else rd.take(1)
                for c in range(4 if ab else 3):
                    ends[s][e][c] = (ends[s][e][c] << 1) | p
        precision = [cb + 1, cb + 1, cb + 1, ab + 1 if ab else 0]
    for s in range(ns):
        for e in range(2):
            for c in range(4 if ab else 3):
                v, n = ends[s][e][c], precision[c]
                v <<= 8 - n
                ends[s][e][c] = v | (v >> n)
    if ns == 1:
        subsets, anchors = [0] * 16, {0}
    elif ns == 2:
        subsets, anchors = _P2[shape], {0, _A2[shape]}
    else:
        subsets, anchors = _P3[shape], {0, _A3_SECOND[shape], _A3_THIRD[shape]}
    first = _indices(rd, ib, anchors)
    second = _indices(rd, ib2, {0}) if ib2 else None
    assert rd.at == 128
    out = []
    for i in range(16):
        e0, e1 = ends[subsets[i]]
        colour_w, alpha_w = _WEIGHTS[ib][first[i]], _WEIGHTS[ib][first[i]]
        if ib2:
            alpha_w = _WEIGHTS[ib2][second[i]]
            if index_selection:
                colour_w, alpha_w = alpha_w, colour_w
        lerp = lambda a, b, w: ((64 - w) * a + w * b + 32) >> 6
        px = [lerp(e0[c], e1[c], colour_w) for c in range(3)] + [lerp(e0[3], e1[3], alpha_w)]
        if rotation:
            px[rotation - 1], px[3] = px[3], px[rotation - 1]
        out.append(tuple(px))
    return out


# BC6H: the bit stream of every mode, first bit first, as the specification's table lists it.  f[a:b] places bit b first.
# r0 g0 b0 / r1 g1 b1 are the endpoints of the first subset, r2.. / r3.. of the second; d is the partition shape.
_BC6_MODES = {
    0: (10, (5, 5, 5), True, "m[1:0] g2[4] b2[4] b3[4] r0[9:0] g0[9:0] b0[9:0] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    1: (7, (6, 6, 6), True, "m[1:0] g2[5] g3[4] g3[5] r0[6:0] b3[0] b3[1] b2[4] g0[6:0] b2[5] b3[2] g2[4] b0[6:0] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
    2: (11, (5, 4, 4), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[4:0] r0[10] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    6: (11, (4, 5, 4), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] g3[4] g2[3:0] g1[4:0] g0[10] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[3:0] b3[0] b3[2] r3[3:0] g2[4] b3[3] d[4:0]"),
    10: (11, (4, 4, 5), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] b2[4] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[4:0] b0[10] b2[3:0] r2[3:0] b3[1] b3[2] r3[3:0] b3[4] b3[3] d[4:0]"),
    14: (9, (5, 5, 5), True, "m[4:0] r0[8:0] b2[4] g0[8:0] g2[4] b0[8:0] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    18: (8, (6, 5, 5), True, "m[4:0] r0[7:0] g3[4] b2[4] g0[7:0] b3[2] g2[4] b0[7:0] b3[3] b3[4] r1[5:0] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
    22: (8, (5, 6, 5), True, "m[4:0] r0[7:0] b3[0] b2[4] g0[7:0] g2[5] g2[4] b0[7:0] g3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[5:0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    26: (8, (5, 5, 6), True, "m[4:0] r0[7:0] b3[1] b2[4] g0[7:0] b2[5] g2[4] b0[7:0] b3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[5:0] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3] d[4:0]"),
    30: (6, (6, 6, 6), False, "m[4:0] r0[5:0] g3[4] b3[0] b3[1] b2[4] g0[5:0] g2[5] b2[5] b3[2] g2[4] b0[5:0] g3[5] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0] d[4:0]"),
    3: (10, (10, 10, 10), False, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[9:0] g1[9:0] b1[9:0]"),
    7: (11, (9, 9, 9), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[8:0] r0[10] g1[8:0] g0[10] b1[8:0] b0[10]"),
    11: (12, (8, 8, 8), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[7:0] r0[10:11] g1[7:0] g0[10:11] b1[7:0] b0[10:11]"),
    15: (16, (4, 4, 4), True, "m[4:0] r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10:15] g1[3:0] g0[10:15] b1[3:0] b0[10:15]"),
}


def _bc6_fields(block, layout):
    fields, at = {}, 0
    for item in layout.split():
        name, span = item[:-1].split("[")
        a, b = (int(v) for v in span.split(":")) if ":" in span else (int(span), int(span))
        step = 1 if a >= b else -1
        for bit in range(b, a + step, step):
            fields[name] = fields.get(name, 0) | (((block >> at) & 1) << bit)
            at += 1
    return fields, at


def _sext(v, n):
    return v - (1 << n) if v & (1 << (n - 1)) else v


def _bc6_unquantize(v, n, signed):
    if signed:
        v = _sext(v & ((1 << n) - 1), n)
        if n >= 16:
            return v
        s, v = (-1, -v) if v < 0 else (1, v)
        if v == 0:
            u = 0
        elif v >= (1 << (n - 1)) - 1:
            u = 0x7fff
        else:
            u = ((v << 15) + 0x4000) >> (n - 1)
        return s * u
    v &= (1 << n) - 1
    if n >= 15 or v == 0:
        return v
    if v == (1 << n) - 1:
        return 0xffff
    return ((v << 15) + 0x4000) >> (n - 1)


def _bc6(block, signed):
    """16 x (r, g, b, a) as the bits of halves."""
    mode = block & 3 if (block & 3) < 2 else block & 31
    if mode not in _BC6_MODES:
        return [(0, 0, 0, 0x3c00)] * 16  # reserved
    bits, delta, transformed, layout = _BC6_MODES[mode]
    f, at = _bc6_fields(block, layout)
    two = "d" in f
    assert at == (82 if two else 65)
    ends = [[[f["rgb"[c] + str(2 * s + e)] for c in range(3)] for e in range(2)] for s in range(2 if two else 1)]
    if transformed:
        for s in range(len(ends)):
            for e in range(2):
                if s or e:
                    for c in range(3):
                        ends[s][e][c] = ends[0][0][c] + _sext(ends[s][e][c], delta[c])
    ends = [[[_bc6_unquantize(v, bits, signed) for v in e] for e in s] for s in ends]
    subsets, anchors = (_P2[f["d"]], {0, _A2[f["d"]]}) if two else ([0] * 16, {0})
    rd = _Reader(block)
    rd.at = at
    ib = 3 if two else 4
    idx = _indices(rd, ib, anchors)
    assert rd.at == 128
    out = []
    for i in range(16):
        e0, e1 = ends[subsets[i]]
        w = _WEIGHTS[ib][idx[i]]
        px = []
        for c in range(3):
            v = ((64 - w) * e0[c] + w * e1[c] + 32) >> 6
            if signed:
                v = (0x8000 | ((-v * 31) >> 5)) if v < 0 else (v * 31) >> 5
                if v == 0x8000:
                    v = 0  # no negative zero
            else:
                v = (v * 31) >> 6
            px.append(v)
        out.append((px[0], px[1], px[2], 0x3c00))
    return out


# ---- images -----------------------------------------------------------------------------------------------------------------------

def decode_block(fmt, raw):
    """One block (bytes) -> (16 x channels values, 16 x channels tie flags), texel 0 first."""
    lo = int.from_bytes(bytes(raw[:8]), "little")
    hi = int.from_bytes(bytes(raw[8:16]), "little") if len(raw) > 8 else 0
    if fmt in (BC1_RGB_UNORM, BC1_RGB_SRGB, BC1_RGBA_UNORM, BC1_RGBA_SRGB):
        rgba = fmt in (BC1_RGBA_UNORM, BC1_RGBA_SRGB)
        px = _bc1_colours(lo, False, 0 if rgba else 255)
        return [p[0] for p in px], [p[1] for p in px]
    if fmt in (BC2_UNORM, BC2_SRGB, BC3_UNORM, BC3_SRGB):
        px = _bc1_colours(hi, True, 255)
        alpha = [(((lo >> (4 * i)) & 15) * 17, False) for i in range(16)] if fmt in (BC2_UNORM, BC2_SRGB) else _rgtc(lo)
        return [p[0][:3] + [a[0]] for p, a in zip(px, alpha)], [p[1][:3] + [a[1]] for p, a in zip(px, alpha)]
    if fmt == BC4_UNORM:
        r = _rgtc(lo)
        return [[v[0]] for v in r], [[v[1]] for v in r]
    if fmt == BC5_UNORM:
        r, g = _rgtc(lo), _rgtc(hi)
        return [[a[0], b[0]] for a, b in zip(r, g)], [[a[1], b[1]] for a, b in zip(r, g)]
    block = lo | (hi << 64)
    if fmt in (BC7_UNORM, BC7_SRGB):
        px = _bc7(block)
    elif fmt in (BC6H_UFLOAT, BC6H_SFLOAT):
        px = _bc6(block, fmt == BC6H_SFLOAT)
    else:
        raise ValueError(f"format {fmt} is not BC1-BC7")
    return [list(p) for p in px], [[False] * 4] * 16


def decode(fmt, blocks, width, height):
    """blocks: uint8 array of ceil(height/4) x ceil(width/4) blocks (any shape with that many bytes, row-major).
    Returns (image, ties): image (height, width[, channels]) and a boolean array of the same shape."""
    bw, bh, nb = (width + 3) // 4, (height + 3) // 4, BLOCK_BYTES[fmt]
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(bh, bw, nb)
    channels, dtype = DECODED.get(fmt, (4, np.uint8))
    image = np.zeros((bh * 4, bw * 4, channels), dtype)
    ties = np.zeros((bh * 4, bw * 4, channels), bool)
    for by in range(bh):
        for bx in range(bw):
            values, flags = decode_block(fmt, blocks[by, bx])
            image[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = np.array(values, dtype).reshape(4, 4, channels)
            ties[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = np.array(flags, bool).reshape(4, 4, channels)
    image, ties = image[:height, :width], ties[:height, :width]
    if channels == 1:
        image, ties = image[..., 0], ties[..., 0]
    return np.ascontiguousarray(image), np.ascontiguousarray(ties)
