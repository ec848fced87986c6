"""TEST INFRASTRUCTURE.  A NumPy decoder of ASTC LDR blocks (2-D footprints) written from the format's specification (Khronos Data
Format Specification, ASTC chapter) and, where the reference's decode shader departs from it, from the shader
(assets/shaders/decode/astc.comp with DECODE_8BIT): endpoints are expanded to (c << 8) | 0x80, interpolated in 16 bits and the top byte is
stored, for UNORM and SRGB alike; the error colour (255, 0, 255, 255) is a property of a texel, so the texels of an LDR partition decode
where another partition of the block has an HDR endpoint mode; a void extent stores the top bytes of its colour and its HDR flag is not
looked at.  It does not share a line with granite_amd/csrc/astc_decode.hpp: blocks are decoded all at once, a header field is an array
over blocks, and the tables are built here from the specification's rules.

decode(fmt or (bw, bh), blocks, width, height) -> (height, width, 4) uint8.  tests/test_astc_ref_cpu.py holds it to the executed shader
(tests/golden/astc_decode_shader_v1.npz) byte for byte; the GPU tests use it for the sizes the golden does not hold."""
import numpy as np

FOOTPRINTS = ((4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12))
ERROR_COLOUR = (255, 0, 255, 255)
LDR_MODES = (0, 1, 4, 5, 6, 8, 9, 10, 12, 13)
HDR_MODES = (2, 3, 7, 11, 14, 15)

# (bits, trits, quints): endpoint quantisers from 256 levels down to 6, weight quantisers by range index (None: reserved)
ENDPOINT_QUANTS = ((8, 0, 0), (6, 1, 0), (5, 0, 1), (7, 0, 0), (5, 1, 0), (4, 0, 1), (6, 0, 0), (4, 1, 0), (3, 0, 1), (5, 0, 0), (3, 1, 0),
                   (2, 0, 1), (4, 0, 0), (2, 1, 0), (1, 0, 1), (3, 0, 0), (1, 1, 0))
WEIGHT_QUANTS = (None, None, (1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 1), (1, 1, 0), (3, 0, 0), None, None, (1, 0, 1), (2, 1, 0), (4, 0, 0),
                 (2, 0, 1), (3, 1, 0), (5, 0, 0))


def format_footprint(fmt):
    """VkFormat 157 ... 184 -> (block width, block height)."""
    if not 157 <= fmt <= 184:
        raise ValueError(f"format {fmt} is not an ASTC LDR format")
    return FOOTPRINTS[(fmt - 157) // 2]


def sequence_bits(quant, count):
    """Bits an integer sequence of `count` values takes."""
    b, t, q = quant
    return b * count + (8 * count * t + 4) // 5 + (7 * count * q + 2) // 3


def levels(quant):
    b, t, q = quant
    return (1 << b) * (3 if t else 1) * (5 if q else 1)


def _replicate(value, nbits, width):
    out, have = 0, 0
    while have < width:
        out, have = (out << nbits) | value, have + nbits
    return out >> (have - width)


def unquantise_endpoint(quant, value):
    b, t, q = quant
    if not t and not q:
        return _replicate(value, b, 8)
    bit = [(value >> i) & 1 for i in range(6)]
    a = 0x1ff if bit[0] else 0
    d = value >> b
    if t:
        c = (204, 93, 44, 22, 11, 5)[b - 1]
        bb = (0, bit[1] * 0b100010110, bit[1] * 0b010000101 + bit[2] * 0b100001010, bit[1] * 0b001000001 + bit[2] * 0b010000010 + bit[3] * 0b100000100,
              bit[1] * 0b000100000 + bit[2] * 0b001000000 + bit[3] * 0b010000001 + bit[4] * 0b100000010,
              bit[1] * 0b000010000 + bit[2] * 0b000100000 + bit[3] * 0b001000000 + bit[4] * 0b010000000 + bit[5] * 0b100000001)[b - 1]
    else:
        c = (113, 54, 26, 13, 6)[b - 1]
        bb = (0, bit[1] * 0b100001100, bit[1] * 0b010000010 + bit[2] * 0b100000101, bit[1] * 0b001000000 + bit[2] * 0b010000001 + bit[3] * 0b100000010,
              bit[1] * 0b000100000 + bit[2] * 0b001000000 + bit[3] * 0b010000000 + bit[4] * 0b100000001)[b - 1]
    v = (d * c + bb) ^ a
    return (a & 0x80) | (v >> 2)


def unquantise_weight(quant, value):
    b, t, q = quant
    if not t and not q:
        w = _replicate(value, b, 6)
    elif b == 0:
        w = (0, 32, 63)[value] if t else (0, 16, 32, 47, 63)[value]
    else:
        bit = [(value >> i) & 1 for i in range(3)]
        a = 0x7f if bit[0] else 0
        d = value >> b
        if t:
            c = (50, 23, 11)[b - 1]
            bb = (0, bit[1] * 0b1000101, bit[1] * 0b0100001 + bit[2] * 0b1000010)[b - 1]
        else:
            c = (28, 13)[b - 1]
            bb = (0, bit[1] * 0b1000010)[b - 1]
        v = (d * c + bb) ^ a
        w = (a & 0x20) | (v >> 2)
    return w + 1 if w > 32 else w


def trits_of(T):
    """The five trits packed in 8 bits (the specification's decode of T)."""
    if (T >> 2) & 7 == 7:
        C = ((T >> 5) << 2) | (T & 3)
        t4 = t3 = 2
    else:
        C = T & 0x1f
        if (T >> 5) & 3 == 3:
            t4, t3 = 2, T >> 7
        else:
            t4, t3 = T >> 7, (T >> 5) & 3
    if C & 3 == 3:
        t2, t1, t0 = 2, C >> 4, (((C >> 3) & 1) << 1) | (((C >> 2) & 1) & ~((C >> 3) & 1) & 1)
    elif (C >> 2) & 3 == 3:
        t2, t1, t0 = 2, 2, C & 3
    else:
        t2, t1, t0 = C >> 4, (C >> 2) & 3, (((C >> 1) & 1) << 1) | ((C & 1) & ~((C >> 1) & 1) & 1)
    return t0, t1, t2, t3, t4


def quints_of(Q):
    """The three quints packed in 7 bits."""
    if (Q >> 1) & 3 == 3 and (Q >> 5) & 3 == 0:
        q2 = ((Q & 1) << 2) | ((((Q >> 4) & 1) & ~Q & 1) << 1) | (((Q >> 3) & 1) & ~Q & 1)
        return 4, 4, q2
    if (Q >> 1) & 3 == 3:
        q2, C = 4, (((Q >> 3) & 3) << 3) | ((~(Q >> 5) & 3) << 1) | (Q & 1)
    else:
        q2, C = (Q >> 5) & 3, Q & 0x1f
    if C & 7 == 5:
        return (C >> 3) & 3, 4, q2
    return C & 7, (C >> 3) & 3, q2


def block_mode(mode):
    """The 11 block-mode bits -> (layout 0..9 or None when reserved, grid width, grid height, weight range index, dual plane).
    Layouts in the order of the specification's table; a reserved weight range (index < 2 of its low three bits) is not a reserved
    layout here: the range index comes back as it is coded."""
    bit = lambda i, n=1: (mode >> i) & ((1 << n) - 1)
    a, b, dual, high = bit(5, 2), bit(7, 2), bit(10), bit(9)
    if mode & 3:
        r = bit(4) | (bit(0, 2) << 1) | (high << 3)
        sel = bit(2, 2)
        if sel == 0:
            return 0, b + 4, a + 2, r, dual
        if sel == 1:
            return 1, b + 8, a + 2, r, dual
        if sel == 2:
            return 2, a + 2, b + 8, r, dual
        if b & 2:
            return 4, (b & 1) + 2, a + 2, r, dual
        return 3, a + 2, (b & 1) + 6, r, dual
    r = bit(4) | (bit(2, 2) << 1) | (high << 3)
    if b == 0:
        return 5, 12, a + 2, r, dual
    if b == 1:
        return 6, a + 2, 12, r, dual
    if b == 2:
        return 9, a + 6, bit(9, 2) + 6, r & 7, 0
    if a == 0:
        return 7, 6, 10, r, dual
    if a == 1:
        return 8, 10, 6, r, dual
    return None, 0, 0, r, dual


def hash52(p):
    m = 0xffffffff
    p ^= p >> 15
    p = (p - (p << 17)) & m
    p = (p + (p << 7)) & m
    p = (p + (p << 4)) & m
    p ^= p >> 5
    p = (p + (p << 16)) & m
    p ^= p >> 7
    p ^= p >> 3
    p = (p ^ (p << 6)) & m
    p ^= p >> 17
    return p


def select_partition(seed, x, y, count, small):
    """The specification's partition function for a 2-D block (z = 0)."""
    if small:
        x, y = x << 1, y << 1
    seed += (count - 1) * 1024
    rnum = hash52(seed)
    s = [(rnum >> sh) & 0xf for sh in (0, 4, 8, 12, 16, 20, 24, 28)]
    s = [v * v for v in s]
    if seed & 1:
        sh1, sh2 = (4 if seed & 2 else 5), (6 if count == 3 else 5)
    else:
        sh1, sh2 = (6 if count == 3 else 5), (4 if seed & 2 else 5)
    s = [v >> (sh2 if i & 1 else sh1) for i, v in enumerate(s)]
    a = (s[0] * x + s[1] * y + (rnum >> 14)) & 0x3f
    b = (s[2] * x + s[3] * y + (rnum >> 10)) & 0x3f
    c = (s[4] * x + s[5] * y + (rnum >> 6)) & 0x3f if count >= 3 else 0
    d = (s[6] * x + s[7] * y + (rnum >> 2)) & 0x3f if count >= 4 else 0
    if a >= b and a >= c and a >= d:
        return 0
    if b >= c and b >= d:
        return 1
    return 2 if c >= d else 3


_CACHE = {}


def tables():
    """The lookup tables in the layout of the shader's buffers: endpoint_quantiser u16 (9, 128, 4) = bits, trits, quints, offset into
    endpoint_unquant; weight_quantiser u8 (16, 4) likewise; trits_quints u16 (384,): five 3-bit trits of T, three 3-bit quints of Q at
    256 + Q."""
    if "tables" not in _CACHE:
        ep_offsets, ep_unquant = [], []
        for quant in ENDPOINT_QUANTS:
            ep_offsets.append(len(ep_unquant))
            ep_unquant += [unquantise_endpoint(quant, v) for v in range(levels(quant))]
        ep_quantiser = np.zeros((9, 128, 4), np.uint16)
        for pairs in range(1, 10):
            for remaining in range(128):
                for i, quant in enumerate(ENDPOINT_QUANTS):
                    if sequence_bits(quant, 2 * pairs) <= remaining:
                        ep_quantiser[pairs - 1, remaining] = (*quant, ep_offsets[i])
                        break
        w_quantiser, w_unquant = np.zeros((16, 4), np.uint8), []
        for i, quant in enumerate(WEIGHT_QUANTS):
            w_quantiser[i] = (*(quant or (0, 0, 0)), len(w_unquant))
            if quant:
                w_unquant += [unquantise_weight(quant, v) for v in range(levels(quant))]
        tq = [sum(t << (3 * i) for i, t in enumerate(trits_of(T))) for T in range(256)] + [sum(q << (3 * i) for i, q in enumerate(quints_of(Q))) for Q in range(128)]
        modes = np.array([[-1 if m[0] is None else m[0], *m[1:]] for m in map(block_mode, range(2048))], np.int64)
        _CACHE["tables"] = {"endpoint_quantiser": ep_quantiser, "endpoint_unquant": np.array(ep_unquant, np.uint8), "weight_quantiser": w_quantiser,
                            "weight_unquant": np.array(w_unquant, np.uint8), "trits_quints": np.array(tq, np.uint16), "block_modes": modes}
    return _CACHE["tables"]


def partition_table(bw, bh):
    """u8 (32 * bh, 32 * bw): partition of (x, y) for 2, 3 and 4 partitions in bits 0-1, 2-3, 4-5, seed s at column s & 31, row s >> 5."""
    key = ("partition", bw, bh)
    if key not in _CACHE:
        # select_partition for every seed and texel at once: seed, y, x along three axes
        seed = np.arange(1024, dtype=np.int64)[:, None, None]
        scale = 2 if bw * bh < 31 else 1
        y, x = np.arange(bh, dtype=np.int64)[None, :, None] * scale, np.arange(bw, dtype=np.int64)[None, None, :] * scale
        packed = np.zeros((1024, bh, bw), np.int64)
        for count in (2, 3, 4):
            rnum = np.array([hash52(s + (count - 1) * 1024) for s in range(1024)], np.int64)[:, None, None]
            odd, bit1 = (seed & 1) == 1, (seed & 2) == 2
            sh1 = np.where(odd, np.where(bit1, 4, 5), 6 if count == 3 else 5)
            sh2 = np.where(odd, 6 if count == 3 else 5, np.where(bit1, 4, 5))
            s = [(((rnum >> (4 * i)) & 0xf) ** 2) >> (sh2 if i & 1 else sh1) for i in range(8)]
            a = (s[0] * x + s[1] * y + (rnum >> 14)) & 0x3f
            b = (s[2] * x + s[3] * y + (rnum >> 10)) & 0x3f
            c = (s[4] * x + s[5] * y + (rnum >> 6)) & 0x3f if count >= 3 else np.zeros_like(a)
            d = (s[6] * x + s[7] * y + (rnum >> 2)) & 0x3f if count >= 4 else np.zeros_like(a)
            part = np.where((a >= b) & (a >= c) & (a >= d), 0, np.where((b >= c) & (b >= d), 1, np.where(c >= d, 2, 3)))
            packed |= part << (2 * count - 4)
        _CACHE[key] = np.ascontiguousarray(packed.reshape(32, 32, bh, bw).transpose(0, 2, 1, 3).reshape(32 * bh, 32 * bw).astype(np.uint8))
    return _CACHE[key]


# ---- all blocks at once ----------------------------------------------------------------------------------------------------------------

def _bits(lo, hi, off, n):
    """n (array or int, 0..32) bits from bit off (array or int, >= 0) of the 128-bit blocks (lo, hi: uint64 arrays); 0 beyond bit 127."""
    off = np.broadcast_to(np.asarray(off, np.int64), lo.shape)
    n = np.broadcast_to(np.asarray(n, np.int64), lo.shape)
    o = np.clip(off, 0, 127)
    low = o < 64
    zero = np.zeros_like(lo)
    part = np.where(low, lo >> np.where(low, o, 0).astype(np.uint64), zero)
    carry = np.where(low & (o > 0), hi << np.where(low & (o > 0), 64 - o, 0).astype(np.uint64), zero)
    high = np.where(~low, hi >> np.where(~low, o - 64, 0).astype(np.uint64), zero)
    v = part | carry | high
    mask = (np.uint64(1) << np.clip(n, 0, 32).astype(np.uint64)) - np.uint64(1)
    return np.where((off < 128) & (n > 0), v & mask, zero).astype(np.int64)


def _keep_low(lo, hi, n):
    n = np.asarray(n, np.int64)
    ones = np.uint64(0xffffffffffffffff)
    m_lo = np.where(n >= 64, ones, (np.uint64(1) << np.clip(n, 0, 63).astype(np.uint64)) - np.uint64(1))
    m_hi = np.where(n >= 128, ones, (np.uint64(1) << np.clip(n - 64, 0, 63).astype(np.uint64)) - np.uint64(1))
    return lo & m_lo, hi & np.where(n > 64, m_hi, np.uint64(0))


def _reverse64(v):
    out = np.zeros_like(v)
    for i in range(64):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(63 - i)
    return out


def _sequence_value(lo, hi, start, index, b, trits, quints):
    """Value `index` of the integer sequences that start at bit `start`; b, trits, quints: per-block quantiser."""
    tq = tables()["trits_quints"].astype(np.int64)
    # trits: five values share 8 bits T, spread between the values' own bits
    group, at = index // 5, index % 5
    s = start + group * (5 * b + 8)
    T = _bits(lo, hi, s + b, 2) | (_bits(lo, hi, s + 2 * b + 2, 2) << 2) | (_bits(lo, hi, s + 3 * b + 4, 1) << 4) | \
        (_bits(lo, hi, s + 4 * b + 5, 2) << 5) | (_bits(lo, hi, s + 5 * b + 7, 1) << 7)
    own = s + at * b + np.array([0, 2, 4, 5, 7])[at]
    as_trit = (((tq[T] >> (3 * at)) & 7) << b) | _bits(lo, hi, own, b)
    # quints: three values share 7 bits Q
    group, at = index // 3, index % 3
    s = start + group * (3 * b + 7)
    Q = _bits(lo, hi, s + b, 3) | (_bits(lo, hi, s + 2 * b + 3, 2) << 3) | (_bits(lo, hi, s + 3 * b + 5, 2) << 5)
    own = s + at * b + np.array([0, 3, 5])[at]
    as_quint = (((tq[256 + Q] >> (3 * at)) & 7) << b) | _bits(lo, hi, own, b)
    plain = _bits(lo, hi, start + index * b, b)
    return np.where(trits > 0, as_trit, np.where(quints > 0, as_quint, plain))


def _bit_transfer_signed(a, b):
    b = (b >> 1) | (a & 0x80)
    a = (a >> 1) & 0x3f
    return np.where(a & 0x20, a - 0x40, a), b


def _endpoints(mode, v):
    """mode: (B,), v: (B, 8) unquantised values -> e0, e1 (B, 4) and whether the mode is an LDR one."""
    B = mode.shape[0]
    e0, e1 = np.zeros((B, 4), np.int64), np.zeros((B, 4), np.int64)
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[:, i] for i in range(8))
    full = np.full(B, 255, np.int64)

    def put(which, a, b):
        e0[which], e1[which] = np.stack(a, 1)[which], np.stack(b, 1)[which]

    put(mode == 0, (v0, v0, v0, full), (v1, v1, v1, full))
    l0 = (v0 >> 2) | (v1 & 0xc0)
    l1 = np.minimum(l0 + (v1 & 0x3f), 255)
    put(mode == 1, (l0, l0, l0, full), (l1, l1, l1, full))
    put(mode == 4, (v0, v0, v0, v2), (v1, v1, v1, v3))
    o1, b0 = _bit_transfer_signed(v1, v0)
    o3, b2 = _bit_transfer_signed(v3, v2)
    put(mode == 5, (b0, b0, b0, b2), (b0 + o1, b0 + o1, b0 + o1, b2 + o3))
    put(mode == 6, ((v0 * v3) >> 8, (v1 * v3) >> 8, (v2 * v3) >> 8, full), (v0, v1, v2, full))
    put(mode == 10, ((v0 * v3) >> 8, (v1 * v3) >> 8, (v2 * v3) >> 8, v4), (v0, v1, v2, v5))
    for m, a0, a1 in ((8, full, full), (12, v6, v7)):
        keep = v1 + v3 + v5 >= v0 + v2 + v4
        put((mode == m) & keep, (v0, v2, v4, a0), (v1, v3, v5, a1))
        put((mode == m) & ~keep, ((v1 + v5) >> 1, (v3 + v5) >> 1, v5, a1), ((v0 + v4) >> 1, (v2 + v4) >> 1, v4, a0))
    o1, b0 = _bit_transfer_signed(v1, v0)
    o3, b2 = _bit_transfer_signed(v3, v2)
    o5, b4 = _bit_transfer_signed(v5, v4)
    o7, b6 = _bit_transfer_signed(v7, v6)
    for m, a0, a1 in ((9, full, full), (13, b6, b6 + o7)):
        keep = o1 + o3 + o5 >= 0
        put((mode == m) & keep, (b0, b2, b4, a0), (b0 + o1, b2 + o3, b4 + o5, a1))
        put((mode == m) & ~keep, ((b0 + o1 + b4 + o5) >> 1, (b2 + o3 + b4 + o5) >> 1, b4 + o5, a1), ((b0 + b4) >> 1, (b2 + b4) >> 1, b4, a0))
    return np.clip(e0, 0, 255), np.clip(e1, 0, 255), np.isin(mode, LDR_MODES)


def decode_blocks(blocks, bw, bh):
    """blocks: (..., 16) uint8 -> (N, bh, bw, 4) uint8, every texel of every block."""
    t = tables()
    raw = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    lo, hi = raw[:, :8].copy().view("<u8")[:, 0], raw[:, 8:].copy().view("<u8")[:, 0]
    B = lo.shape[0]
    out = np.zeros((B, bh, bw, 4), np.uint8)
    if B == 0:
        return out
    bits = lambda off, n: _bits(lo, hi, off, n)

    # void extent
    void = bits(0, 9) == 0x1fc
    ext = [bits(12 + 13 * i, 13) for i in range(4)]
    all_ones = np.logical_and.reduce([e == 0x1fff for e in ext])
    void_error = (bits(10, 2) != 3) | (~all_ones & ((ext[0] >= ext[1]) | (ext[2] >= ext[3])))
    void_colour = np.stack([bits(64 + 16 * c, 16) >> 8 for c in range(4)], 1)

    # block mode
    layout, gw, gh, wrange, dual = (t["block_modes"][bits(0, 11)][:, i] for i in range(5))
    parts = bits(11, 2) + 1
    error = (layout < 0) | (gw > bw) | (gh > bh) | ((dual == 1) & (parts == 4))
    wq = t["weight_quantiser"].astype(np.int64)[wrange]
    count = gw * gh * (1 + dual)
    wbits = wq[:, 0] * count + (8 * count * wq[:, 1] + 4) // 5 + (7 * count * wq[:, 2] + 2) // 3
    error |= (count > 64) | (wbits < 24) | (wbits > 96)
    wbits = np.clip(wbits, 0, 96)

    # colour endpoint modes
    multi = parts > 1
    cem = np.where(multi, bits(23, 6), bits(13, 4))
    separate = multi & ((cem & 3) != 0)
    extra = np.where(separate, 3 * parts - 4, 0)
    field = (bits(128 - wbits - extra, extra) << 4) | (cem >> 2)
    mode, base = np.zeros((B, 4), np.int64), np.zeros((B, 4), np.int64)
    pairs = np.zeros(B, np.int64)
    for p in range(4):
        cls = (cem & 3) - 1 + ((field >> p) & 1)
        m = np.where(separate, 4 * cls + ((field >> (parts + 2 * p)) & 3), np.where(multi, cem >> 2, cem))
        live = p < parts
        mode[:, p], base[:, p] = np.where(live, m, 0), 2 * pairs
        pairs = pairs + np.where(live, (m >> 2) + 1, 0)
    config = np.where(multi, np.where(separate, 25 + 3 * parts, 29), 17) + 2 * dual
    start = np.where(multi, 29, 17)
    remaining = np.clip(128 - config - wbits, 0, 127)
    error |= pairs > 9
    eq = t["endpoint_quantiser"].astype(np.int64)[np.clip(pairs, 1, 9) - 1, remaining]
    error |= (eq[:, :3] == 0).all(1)
    e_lo, e_hi = _keep_low(lo, hi, start + eq[:, 0] * 2 * pairs + (16 * pairs * eq[:, 1] + 4) // 5 + (14 * pairs * eq[:, 2] + 2) // 3)
    unq = np.concatenate([t["endpoint_unquant"].astype(np.int64), np.zeros(64, np.int64)])
    values = np.stack([unq[eq[:, 3] + _sequence_value(e_lo, e_hi, start, np.full(B, i), eq[:, 0], eq[:, 1], eq[:, 2])] for i in range(18)] + [np.zeros(B, np.int64)] * 8, 1)
    e0, e1, ldr = np.zeros((B, 4, 4), np.int64), np.zeros((B, 4, 4), np.int64), np.zeros((B, 4), bool)
    for p in range(4):
        v = np.take_along_axis(values, np.clip(base[:, p], 0, 18)[:, None] + np.arange(8)[None, :], 1)
        e0[:, p], e1[:, p], ldr[:, p] = _endpoints(mode[:, p], v)

    # weights, read from the top of the block down
    r_lo, r_hi = _keep_low(_reverse64(hi), _reverse64(lo), wbits)
    wunq = np.concatenate([t["weight_unquant"].astype(np.int64), np.zeros(64, np.int64)])
    weights = np.stack([wunq[wq[:, 3] + _sequence_value(r_lo, r_hi, 0, np.full(B, i), wq[:, 0], wq[:, 1], wq[:, 2])] for i in range(64)] + [np.zeros(B, np.int64)] * 64, 1)
    plane2 = bits(126 - wbits - extra, 2)
    seed = bits(13, 10)
    ptable = partition_table(bw, bh).astype(np.int64)
    rows = np.arange(B)
    stride = 1 + dual

    for y in range(bh):
        for x in range(bw):
            packed = ptable[(seed >> 5) * bh + y, (seed & 31) * bw + x]
            part = np.where(multi, (packed >> np.clip(2 * parts - 4, 0, 4)) & 3, 0)
            # the texel's place in the weight grid, 4 fractional bits
            fx = ((((1024 + bw // 2) // (bw - 1)) * x * (gw - 1) + 32) >> 6)
            fy = ((((1024 + bh // 2) // (bh - 1)) * y * (gh - 1) + 32) >> 6)
            tx, ty, at = fx & 15, fy & 15, (fy >> 4) * gw + (fx >> 4)
            w11 = (tx * ty + 8) >> 4
            factors = ((16 - tx - ty + w11, at), (tx - w11, at + 1), (ty - w11, at + gw), (w11, at + gw + 1))
            plane = []
            for k in range(2):
                acc = np.full(B, 8, np.int64)
                for factor, index in factors:
                    acc = acc + factor * weights[rows, np.clip(index * stride + k, 0, 127)]  # a factor of 0 where the neighbour lies outside the grid
                plane.append(acc >> 4)
            for c in range(4):
                w = np.where((dual == 1) & (plane2 == c), plane[1], plane[0])
                c0, c1 = (e0[rows, part, c] << 8) | 0x80, (e1[rows, part, c] << 8) | 0x80
                texel = ((c0 * (64 - w) + c1 * w + 32) >> 6) >> 8
                texel = np.where(error | ~ldr[rows, part], ERROR_COLOUR[c], texel)
                texel = np.where(void, np.where(void_error, ERROR_COLOUR[c], void_colour[:, c]), texel)
                out[:, y, x, c] = texel
    return out


def assemble(texels, bw, bh, width, height):
    """(rows of blocks * blocks per row, bh, bw, 4) decoded blocks -> the (height, width, 4) image they tile."""
    bx, by = (width + bw - 1) // bw, (height + bh - 1) // bh
    return np.ascontiguousarray(texels.reshape(by, bx, bh, bw, 4).transpose(0, 2, 1, 3, 4).reshape(by * bh, bx * bw, 4)[:height, :width])


def decode(fmt, blocks, width, height):
    """blocks: (rows of blocks, blocks per row, 16) or anything of that many bytes -> (height, width, 4) uint8.  fmt: a VkFormat or (bw, bh)."""
    bw, bh = fmt if isinstance(fmt, tuple) else format_footprint(fmt)
    bx, by = (width + bw - 1) // bw, (height + bh - 1) // bh
    return assemble(decode_blocks(np.ascontiguousarray(blocks, np.uint8).reshape(by * bx, 16), bw, bh), bw, bh, width, height)
