"""TEST INFRASTRUCTURE.  The block sets the ASTC decode tests share.  Blocks are built, not filtered: a random 128-bit payload gets the
header fields of its class forced into it (block mode, partition count and seed, CEM field(s) with their extra bits below the weights,
void-extent fields), the block mode being drawn from the encodings of astc_ref.block_mode that meet the class's conditions for the
footprint.  cases() -> {name: (format, width, height, blocks)} generates them (tests/golden/make_astc_decode_golden.py records them);
golden() -> {name: (format, width, height, blocks, out)} reads them back with what the reference's decode shader, executed on the CPU,
stored for them (tests/golden/astc_decode_shader_v1.npz).

A case is `f<bw>x<bh>_<class>`; a class whose name starts with `err_` is an error class: every one of its blocks holds at least one
texel of the error colour.  In every other class at most a quarter of the blocks may hold one (they hold none: the construction keeps
them legal).  Two classes the shader settles otherwise than the words "error cause" suggest: `void_hdr` (the HDR flag of a void extent)
is no error in the shader's 8-bit mode, so it is not an error class; and a layout of the block-mode table whose grids are all larger
than the footprint is the error class `err_layout<k>` there and the legal class `layout<k>` where a grid fits.
The full matrix runs at 4 x 4, 8 x 8 and 12 x 12; the other footprints get partitions x single / dual plane; every footprint gets the
tail sizes."""
import os

import numpy as np

import astc_ref

FULL = ((4, 4), (8, 8), (12, 12))
PER_CLASS = {(4, 4): 32, (8, 8): 16, (12, 12): 12}
ROW = 4  # blocks to a row of a case's image


def astc_format(bw, bh, srgb=False):
    return 157 + 2 * astc_ref.FOOTPRINTS.index((bw, bh)) + int(srgb)


def tail_sizes(bw, bh):
    return ((1, 1), (bw - 1, bh - 1), (bw + 1, bh + 1), (2 * bw + 1, bh + 2))


def _set(value, off, n, field):
    return (value & ~(((1 << n) - 1) << off)) | ((int(field) & ((1 << n) - 1)) << off)


MIN_ENDPOINT_QUANT = astc_ref.ENDPOINT_QUANTS[-1]


class Builder:
    def __init__(self, rng, bw, bh):
        self.rng, self.bw, self.bh = rng, bw, bh
        self.modes = [(m,) + astc_ref.block_mode(m) for m in range(2048) if (m & 0x1ff) != 0x1fc]
        self._full_seeds = {}

    def full_seeds(self, parts):
        """Seeds whose partitions all hold a texel of the footprint."""
        if parts not in self._full_seeds:
            table = (astc_ref.partition_table(self.bw, self.bh) >> (2 * parts - 4)) & 3
            self._full_seeds[parts] = [s for s in range(1024) if len(np.unique(
                table[(s >> 5) * self.bh:(s >> 5) * self.bh + self.bh, (s & 31) * self.bw:(s & 31) * self.bw + self.bw])) == parts]
        return self._full_seeds[parts]

    def random_bits(self):
        return int.from_bytes(self.rng.bytes(16), "little")

    def weight_bits(self, gw, gh, r, dual):
        quant = astc_ref.WEIGHT_QUANTS[r]
        return astc_ref.sequence_bits(quant, gw * gh * (1 + dual)) if quant else 0

    def legal_modes(self, pairs, parts, separate, want=lambda *a: True):
        """Block modes that fit the footprint, have a legal weight range, count and size, and leave the endpoints at least their
        coarsest quantiser."""
        out = []
        for m, layout, gw, gh, r, dual in self.modes:
            if pairs > 9:
                break
            if layout is None or gw > self.bw or gh > self.bh or astc_ref.WEIGHT_QUANTS[r] is None or (dual and parts == 4):
                continue
            count, wbits = gw * gh * (1 + dual), self.weight_bits(gw, gh, r, dual)
            config = (17 if parts == 1 else 25 + 3 * parts if separate else 29) + 2 * dual
            if count > 64 or not 24 <= wbits <= 96 or 128 - config - wbits < astc_ref.sequence_bits(MIN_ENDPOINT_QUANT, 2 * pairs):
                continue
            if want(layout, gw, gh, r, dual, 128 - config - wbits):
                out.append(m)
        return out

    def block(self, cems, mode=None, want=lambda *a: True, separate=None, seed=None):
        """A block with one endpoint mode per partition.  `separate`: code the modes per partition even where they are equal."""
        parts = len(cems)
        classes = [c >> 2 for c in cems]
        if separate is None:
            separate = parts > 1 and len(set(cems)) > 1
        assert not separate or max(classes) - min(classes) <= 1
        pairs = sum(c + 1 for c in classes)
        if mode is None:
            legal = self.legal_modes(pairs, parts, separate, want)
            if not legal:
                return None
            mode = legal[self.rng.integers(len(legal))]
        _, gw, gh, r, dual = astc_ref.block_mode(mode)
        v = _set(self.random_bits(), 0, 11, mode)
        v = _set(v, 11, 2, parts - 1)
        if parts == 1:
            return _set(v, 13, 4, cems[0])
        v = _set(v, 13, 10, self.rng.integers(1024) if seed is None else seed)
        if not separate:
            return _set(v, 23, 6, cems[0] << 2)
        low = min(classes)
        if all(c == low for c in classes) and low > 0 and (low == 3 or self.rng.integers(2)):
            low -= 1  # the same classes coded as base + 1: a choice for classes 1 and 2, the only coding of class 3
        field = sum((c - low) << i for i, c in enumerate(classes)) | sum((m & 3) << (parts + 2 * i) for i, m in enumerate(cems))
        v = _set(v, 23, 6, (low + 1) | ((field & 0xf) << 2))
        extra = 3 * parts - 4
        return _set(v, 128 - self.weight_bits(gw, gh, r, dual) - extra, extra, field >> 4)

    def ldr(self, parts=1):
        """One LDR mode for all of `parts` partitions, of a class that keeps the block within 9 endpoint pairs."""
        return [int(self.rng.choice([m for m in astc_ref.LDR_MODES if ((m >> 2) + 1) * parts <= 9]))] * parts

    def ldr_within_a_class_step(self, n):
        """n LDR modes whose classes differ by at most one (what a per-partition CEM field can code), not all equal."""
        while True:
            low = int(self.rng.integers(0, 3))
            modes = [int(self.rng.choice([m for m in astc_ref.LDR_MODES if low <= m >> 2 <= low + 1])) for _ in range(n)]
            if len(set(modes)) > 1:
                return modes

    def void(self, kind):
        v = _set(self.random_bits(), 0, 9, 0x1fc)
        v = _set(v, 9, 1, 1 if kind == "hdr" else 0)
        v = _set(v, 10, 2, int(self.rng.integers(3)) if kind == "reserved" else 3)
        lo_s, hi_s, lo_t, hi_t = (int(x) for x in (*np.sort(self.rng.choice(0x1fff, 2, replace=False)), *np.sort(self.rng.choice(0x1fff, 2, replace=False))))
        if kind == "inverted":
            if self.rng.integers(2):
                lo_s, hi_s = hi_s, lo_s if self.rng.integers(2) else hi_s  # min > max, or min == max
            else:
                lo_t, hi_t = hi_t, lo_t
        elif self.rng.integers(2):
            lo_s = hi_s = lo_t = hi_t = 0x1fff  # "no extent"
        for i, e in enumerate((lo_s, hi_s, lo_t, hi_t)):
            v = _set(v, 12 + 13 * i, 13, e)
        return v


def _pack(values):
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little") for v in values), np.uint8).reshape(-1, 16).copy()


def _image(blocks, bw, bh):
    rows = len(blocks) // ROW
    assert rows * ROW == len(blocks)
    return astc_format(bw, bh), ROW * bw, rows * bh, _pack(blocks).reshape(rows, ROW, 16)


def _full_matrix(out, rng, bw, bh):
    b, n = Builder(rng, bw, bh), PER_CLASS[(bw, bh)]

    def add(name, make):
        def attempt(i):  # a draw of endpoint modes may leave no block mode that meets the class: draw again
            for _ in range(64):
                v = make(i)
                if v is not None:
                    return v
            return None
        blocks = [attempt(i) for i in range(n)]
        if any(v is None for v in blocks):
            assert all(v is None for v in blocks), name
            return False  # nothing of this class exists for the footprint
        out[f"f{bw}x{bh}_{name}"] = _image(blocks, bw, bh)
        return True

    def illegal_mode(pick):
        """A block whose mode is drawn from the encodings `pick` accepts, legal or not."""
        modes = [m for m, layout, gw, gh, r, dual in b.modes if pick(layout, gw, gh, r, dual)]
        return (lambda i: b.block(b.ldr(), mode=modes[rng.integers(len(modes))])) if modes else (lambda i: None)

    add("void_ldr", lambda i: b.void("ldr"))
    add("void_hdr", lambda i: b.void("hdr"))
    add("err_void_reserved", lambda i: b.void("reserved"))
    add("err_void_inverted", lambda i: b.void("inverted"))
    for k in range(10):
        if not add(f"layout{k}", lambda i: b.block(b.ldr(), want=lambda layout, *a: layout == k)):
            add(f"err_layout{k}", illegal_mode(lambda layout, gw, gh, r, dual: layout == k and astc_ref.WEIGHT_QUANTS[r] is not None))
    add("err_reserved_mode", illegal_mode(lambda layout, *a: layout is None))
    add("err_reserved_range", illegal_mode(lambda layout, gw, gh, r, dual: layout is not None and astc_ref.WEIGHT_QUANTS[r] is None))
    for parts in (1, 2, 3):
        add(f"dual_{parts}part", lambda i: b.block(b.ldr(parts), want=lambda layout, gw, gh, r, dual, left: dual == 1))
    for r in range(16):
        if astc_ref.WEIGHT_QUANTS[r]:
            add(f"range{r}", lambda i: b.block(b.ldr(), want=lambda layout, gw, gh, rr, dual, left: rr == r))
    for parts in (1, 2, 3, 4):
        add(f"part{parts}", lambda i: b.block(b.ldr(parts), seed=(i * 1024 // n + int(rng.integers(1024 // n))) if parts > 1 else None))
    for m in astc_ref.LDR_MODES:
        add(f"cem{m}", lambda i: b.block([m] * (1 + i % 2)))
    for m in astc_ref.HDR_MODES:
        add(f"err_hdr_cem{m}", lambda i: b.block([m] * (1 + i % 2)))
    for parts in (2, 3, 4):
        add(f"mixed_cem_{parts}part", lambda i: b.block(b.ldr_within_a_class_step(parts)))
        add(f"same_cem_coded_apart_{parts}part", lambda i: b.block(b.ldr(parts), separate=True))

        def ldr_and_hdr(i, parts=parts):
            while True:  # one HDR mode among LDR ones, classes a step apart at most, on a seed that gives every partition a texel
                modes = [int(rng.choice(range(16))) for _ in range(parts)]
                hdr = [m in astc_ref.HDR_MODES for m in modes]
                if any(hdr) and not all(hdr) and max(m >> 2 for m in modes) - min(m >> 2 for m in modes) <= 1:
                    break
            seeds = b.full_seeds(parts)
            return b.block(modes, separate=True, seed=seeds[rng.integers(len(seeds))])
        add(f"err_ldr_and_hdr_{parts}part", ldr_and_hdr)
    quants = astc_ref.tables()["endpoint_quantiser"]
    for name, column in (("bits", None), ("trits", 1), ("quints", 2)):
        def fits(layout, gw, gh, r, dual, left, pairs, column=column):
            q = quants[pairs - 1, left]
            return (q[1] == 0 and q[2] == 0) if column is None else q[column] == 1

        def make(i, fits=fits):
            parts = 1 + i % 3
            cems = b.ldr(parts)
            pairs = sum((c >> 2) + 1 for c in cems)
            return b.block(cems, want=lambda *a: fits(*a, pairs))
        add(f"endpoint_{name}", make)
    # the error causes (the reserved mode, the void extents and the HDR modes are above)
    add("err_weight_count", illegal_mode(lambda layout, gw, gh, r, dual: layout is not None and gw <= bw and gh <= bh and astc_ref.WEIGHT_QUANTS[r] is not None
                                         and gw * gh * (1 + dual) > 64))
    add("err_weight_bits_low", illegal_mode(lambda layout, gw, gh, r, dual: layout is not None and gw <= bw and gh <= bh and astc_ref.WEIGHT_QUANTS[r] is not None
                                            and b.weight_bits(gw, gh, r, dual) < 24))
    add("err_weight_bits_high", illegal_mode(lambda layout, gw, gh, r, dual: layout is not None and gw <= bw and gh <= bh and astc_ref.WEIGHT_QUANTS[r] is not None
                                             and gw * gh * (1 + dual) <= 64 and b.weight_bits(gw, gh, r, dual) > 96))
    fits_weights = lambda layout, gw, gh, r, dual: layout is not None and gw <= bw and gh <= bh and astc_ref.WEIGHT_QUANTS[r] is not None and \
        gw * gh * (1 + dual) <= 64 and 24 <= b.weight_bits(gw, gh, r, dual) <= 96
    dual_modes = [m for m, *rest in b.modes if fits_weights(*rest) and rest[4] == 1]
    add("err_dual_4part", lambda i: b.block(b.ldr(4), mode=dual_modes[rng.integers(len(dual_modes))]) if dual_modes else None)
    single_modes = [m for m, *rest in b.modes if fits_weights(*rest) and rest[4] == 0]
    add("err_endpoint_count", lambda i: b.block([int(rng.choice((12, 13)))] * (3 + i % 2), mode=single_modes[rng.integers(len(single_modes))]))
    # 16 values need 42 bits at the coarsest quantiser: weights of 58 bits and more leave 128 - 29 - 58 = 41
    tight_modes = [m for m, *rest in b.modes if fits_weights(*rest) and rest[4] == 0 and b.weight_bits(*rest[1:]) >= 58]
    add("err_endpoint_bits", lambda i: b.block([int(rng.choice((12, 13)))] * 2, mode=tight_modes[rng.integers(len(tight_modes))]) if tight_modes else None)


def cases():
    rng = np.random.default_rng(20261019)
    out = {}
    for bw, bh in astc_ref.FOOTPRINTS:
        if (bw, bh) in FULL:
            _full_matrix(out, rng, bw, bh)
        else:
            b = Builder(rng, bw, bh)
            for dual in (0, 1):
                blocks = [b.block(b.ldr(parts), want=lambda layout, gw, gh, r, d, left: d == dual) for parts in (1, 2, 3, 4 - dual) for _ in range(2)]
                out[f"f{bw}x{bh}_parts_{'dual' if dual else 'single'}"] = _image(blocks, bw, bh)
        b = Builder(rng, bw, bh)
        for w, h in tail_sizes(bw, bh):
            bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
            blocks = [b.block(b.ldr(int(rng.integers(1, 4)))) for _ in range(bx * by)]
            out[f"f{bw}x{bh}_tail_{w}x{h}"] = (astc_format(bw, bh), w, h, _pack(blocks).reshape(by, bx, 16))
    return out


def valid_blocks(rng, bw, bh, count):
    """`count` legal blocks of the mix the tail cases use: one to three partitions, any LDR mode, any block mode that fits."""
    b = Builder(rng, bw, bh)
    return _pack([b.block(b.ldr(int(rng.integers(1, 4)))) for _ in range(count)])


def is_error_class(name):
    return "_err_" in name


_GOLDEN = {}
_REFERENCE = {}
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "astc_decode_shader_v1.npz")


def golden():
    if not _GOLDEN:
        with np.load(GOLDEN_PATH) as z:
            for name in sorted({k.split("/")[0] for k in z.files} - {"tables"}):
                fmt, w, h = (int(v) for v in z[name + "/format"])
                _GOLDEN[name] = (fmt, w, h, z[name + "/blocks"], z[name + "/out"])
    return _GOLDEN


def golden_tables():
    with np.load(GOLDEN_PATH) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("tables/")}


def reference(name):
    """astc_ref's image of a golden case.  Computed once, and for all cases of a footprint in one go: the decoder works on all blocks at
    once and a call costs the same for a dozen blocks as for a thousand."""
    if name not in _REFERENCE:
        footprint = astc_ref.format_footprint(golden()[name][0])
        group = [(n, c) for n, c in golden().items() if astc_ref.format_footprint(c[0]) == footprint]
        texels = astc_ref.decode_blocks(np.concatenate([c[3].reshape(-1, 16) for _, c in group]), *footprint)
        at = 0
        for n, (fmt, w, h, blocks, _) in group:
            count = blocks.shape[0] * blocks.shape[1]
            _REFERENCE[n] = astc_ref.assemble(texels[at:at + count], *footprint, w, h)
            at += count
    return _REFERENCE[name]


def error_texels(image):
    return (image == np.array(astc_ref.ERROR_COLOUR, np.uint8)).all(-1)


def blocks_with_error(image, bw, bh):
    """Per block of a (h, w, 4) image: whether any of its texels inside the image is the error colour."""
    h, w = image.shape[:2]
    by, bx = (h + bh - 1) // bh, (w + bw - 1) // bw
    padded = np.zeros((by * bh, bx * bw), bool)
    padded[:h, :w] = error_texels(image)
    return padded.reshape(by, bh, bx, bw).any((1, 3))
