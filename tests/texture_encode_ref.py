"""TEST INFRASTRUCTURE.  A numpy restatement of the two rules of the texture encoder, written from DESIGN.md 7.16 without regard for
speed beyond working on all blocks of an image at once: the RGTC channel-block compressor (integers) and the UNORM8 mip filter (every
operation in fp32, one rounding each).  tests/test_texture_encode_ref_cpu.py holds it to the reference's own code byte for byte
(tests/golden/texture_encode_v1.npz).  Besides the bytes it reports what the bytes do not show: the way a block took through the
compressor and the ties its search met, which the conditions on the case set are stated in."""
import numpy as np

import texture_encode_cases as tc

DIV_7, DIV_5 = 0x100000 // 7, 0x100000 // 5
CANDIDATES = [(lo, hi) for lo in range(15) for hi in range(lo, 15)]  # the search order
FLAT, SMALL_RANGE, KEPT, SWITCHED = 0, 1, 2, 3


def fetch_blocks(image, channel):
    """(by, bx, 16) of one component of an (h, w, c) image: coordinates past the edge read the last column / row."""
    h, w, _ = image.shape
    by, bx = (h + 3) // 4, (w + 3) // 4
    ys = np.minimum(np.arange(4 * by), h - 1)
    xs = np.minimum(np.arange(4 * bx), w - 1)
    padded = image[ys][:, xs, channel]
    return padded.reshape(by, 4, bx, 4).transpose(0, 2, 1, 3).reshape(by, bx, 16)


def _divider(numerator, r):
    return np.where(r > 0, (numerator + (r >> 1)) // np.maximum(r, 1), 0)


def candidate_errors(s):
    """(n, 120): squared error of every (lo, hi) partition of the sorted values s (n, 16)."""
    out = np.zeros((s.shape[0], len(CANDIDATES)), np.int64)
    position = np.arange(16)[None, :]
    for c, (lo, hi) in enumerate(CANDIDATES):
        p_lo, p_hi = s[:, lo:lo + 1], s[:, hi:hi + 1]
        r = p_hi - p_lo
        below = np.minimum(s, p_lo - s)
        above = np.minimum(255 - s, s - p_hi)
        code = ((s - p_lo) * _divider(0x500000, r) + 0x80000) >> 20
        inside = p_lo + ((r * code * DIV_5 + 0x80000) >> 20) - s
        d = np.where(position < lo, below, np.where(position > hi, above, inside))
        out[:, c] = (d * d).sum(axis=1)
    return out


def encode_channel_blocks(texels):
    """texels (n, 16) -> (blocks (n, 8) uint8, info).  info: form (n,), and for searched blocks endpoint_tie (switched, and two candidates of
    different endpoint values share the least error) and incumbent_tie (kept, and some candidate's error equals the 7-weight error)."""
    t = np.asarray(texels, np.int64).reshape(-1, 16)
    n = t.shape[0]
    lo, hi = t.min(axis=1, keepdims=True), t.max(axis=1, keepdims=True)
    r = hi - lo
    position = ((t - lo) * _divider(0x700000, r) + 0x80000) >> 20
    d = lo + ((r * position * DIV_7 + 0x80000) >> 20) - t
    error7 = (d * d).sum(axis=1)
    codes = np.where(position == 7, 0, np.where(position == 0, 1, 8 - position))
    codes = np.where(r == 0, 0, codes)
    e0, e1 = hi[:, 0].copy(), lo[:, 0].copy()
    form = np.where(r[:, 0] == 0, FLAT, np.where(r[:, 0] < 16, SMALL_RANGE, KEPT))

    s = np.sort(t, axis=1)
    errors = candidate_errors(s)
    best = errors.argmin(axis=1)  # the first of equal minima
    least = errors.min(axis=1)
    searched = r[:, 0] >= 16
    switched = searched & (least < error7)
    form = np.where(switched, SWITCHED, form)
    los, his = np.array([c[0] for c in CANDIDATES]), np.array([c[1] for c in CANDIDATES])
    p_lo = np.take_along_axis(s, los[best][:, None], axis=1)
    p_hi = np.take_along_axis(s, his[best][:, None], axis=1)
    divider = _divider(0x500000, p_hi - p_lo)
    q = ((t - p_lo) * divider + 0x80000) >> 20
    inside = np.where(q == 5, 1, np.where(q != 0, q + 1, 0))
    code5 = np.where(t < p_lo, np.where(t < p_lo - t, 6, 0), np.where(t > p_hi, np.where(255 - t < t - p_hi, 7, 1), inside))
    codes = np.where(switched[:, None], code5, codes)
    e0 = np.where(switched, p_lo[:, 0], e0)
    e1 = np.where(switched, p_hi[:, 0], e1)

    bits = (codes.astype(np.uint64) << (3 * np.arange(16, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    blocks = np.zeros((n, 8), np.uint8)
    blocks[:, 0], blocks[:, 1] = e0, e1
    for i in range(6):
        blocks[:, 2 + i] = (bits >> np.uint64(8 * i)) & np.uint64(0xff)

    at_least = errors == least[:, None]
    ends_lo, ends_hi = s[:, los], s[:, his]  # (n, 120)
    other = at_least & ((ends_lo != p_lo) | (ends_hi != p_hi))
    info = {"form": form, "endpoint_tie": switched & other.any(axis=1),
            "incumbent_tie": searched & ~switched & (least == error7)}
    return blocks, info


def encode_image(image, block_format):
    """(by, bx, 8 or 16) uint8 blocks of an (h, w, c) image, and the info of its channel blocks (red ones first, then green)."""
    channels = 2 if block_format == tc.BC5 else 1
    parts, infos = [], []
    for c in range(channels):
        texels = fetch_blocks(image, c)
        blocks, info = encode_channel_blocks(texels.reshape(-1, 16))
        parts.append(blocks.reshape(texels.shape[0], texels.shape[1], 8))
        infos.append(info)
    info = {k: np.concatenate([i[k] for i in infos]) for k in infos[0]}
    return np.concatenate(parts, axis=2), info


# ---- mips --------------------------------------------------------------------------------------------------------------------------
F = np.float32


def _axis(dst, src):
    rescale = F(src) / F(dst)
    coord = (np.arange(dst, dtype=F) + F(0.5)) * rescale - F(0.5)
    base = np.floor(coord)
    i0 = base.astype(np.int64)
    return i0, np.minimum(i0 + 1, src - 1), (coord - base).astype(F)


def _mix(a, b, t):
    return a * (F(1.0) - t) + b * t


def mip_level_float(src):
    """The value of every texel of the next level times 255, before it is rounded: (h', w', c) float32 of (h, w, c) uint8."""
    h, w, _ = src.shape
    dh, dw = max(h >> 1, 1), max(w >> 1, 1)
    x0, x1, wx = _axis(dw, w)
    y0, y1, wy = _axis(dh, h)
    v = src.astype(F) * (F(1.0) / F(255.0))
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = _mix(v[y0][:, x0], v[y0][:, x1], wx)
    bottom = _mix(v[y1][:, x0], v[y1][:, x1], wx)
    out = _mix(top, bottom, wy) * F(255.0)
    assert out.dtype == F
    return out


def round_half_away(v):
    """roundf for v >= 0: the fraction v - floor(v) is exact in fp32, v + 0.5 is not (0.49999997 + 0.5 rounds to 1)."""
    base = np.floor(v)
    return base + (v - base >= F(0.5)).astype(F)


def mip_level(src):
    v = mip_level_float(src)
    assert (v >= 0).all()
    return np.clip(round_half_away(v), 0, 255).astype(np.uint8)


def mip_chain(level0, levels):
    """[level 0, level 1, ...] of (layers, h, w, c) uint8 arrays."""
    out = [np.ascontiguousarray(level0)]
    for _ in range(1, levels):
        out.append(np.stack([mip_level(layer) for layer in out[-1]]))
    return out


def pack_chain(chain, fmt):
    layers, h, w, _ = chain[0].shape
    layout, size = tc.chain_layout(fmt, w, h, layers, len(chain))
    payload = np.zeros(size, np.uint8)
    for (offset, _, _), level in zip(layout, chain):
        payload[offset:offset + level.size] = level.reshape(-1)
    return payload
