"""An image argument in a chosen memory layout, inside guard bytes: what a launcher of the C ABI promises to take (include/granite_hip.h at
gr_image: the pitch covers a row, pitch and pointer are multiples of the texel size) and what capi.DeviceImage never hands it.

LayoutImage has the duck type the capi.Context wrappers use (.desc .width .height .ptr .format .upload() .download()) and owns one
DeviceBuffer holding  front guard | rows at pitch | back guard.  For texel size t on the 256-byte-aligned allocation:

    tight    pointer aligned    pitch w*t                      control: today's results
    wide256  pointer aligned    pitch roundup(w*t, 256) + 256  alignment-gated fast paths stay selected, pitch != w*t
    pad1     pointer aligned    pitch w*t + t                  every other row misaligned at an even width
    off1     pointer base + t   pitch w*t + 3*t                pointer aligned to the texel only

An input is filled with 0x7E (fp16 NaN, fp32 8e37, UNORM8 126: a tap that leaves its row shows in the comparison with the oracle), an
output with 0xA5.  check_guards() asserts that every byte outside the texels still holds its fill, check_unchanged() the same for an input,
texels included.  The bookkeeping needs numpy alone: `buffer` is anything with .ptr, .upload(array, offset) and .download(dtype)
(tests/test_layout_images_cpu.py runs it on a fake)."""
import numpy as np

from granite_amd import capi

LAYOUTS = ("tight", "wide256", "pad1", "off1")
INPUT_FILL, OUTPUT_FILL = 0x7E, 0xA5
GUARD = 256  # bytes in front of and behind the rows; a multiple of 256 so the front guard keeps the allocation's alignment

# format -> (numpy type of a component, components of a texel)
_TEXEL = {
    capi.FORMAT_R16G16B16A16_SFLOAT: (np.uint16, 4),
    capi.FORMAT_R8G8B8A8_SRGB: (np.uint8, 4), capi.FORMAT_R8G8B8A8_UNORM: (np.uint8, 4),
    capi.FORMAT_B8G8R8A8_UNORM: (np.uint8, 4), capi.FORMAT_B8G8R8A8_SRGB: (np.uint8, 4),
    capi.FORMAT_R8_UNORM: (np.uint8, 1), capi.FORMAT_R8G8_UNORM: (np.uint8, 2),
    capi.FORMAT_R16_UNORM: (np.uint16, 1), capi.FORMAT_R16G16_UNORM: (np.uint16, 2),
    capi.FORMAT_R16_SFLOAT: (np.uint16, 1), capi.FORMAT_R16G16_SFLOAT: (np.uint16, 2),
    capi.FORMAT_D32_SFLOAT: (np.float32, 1), capi.FORMAT_R32_SFLOAT: (np.float32, 1),
    capi.FORMAT_A2B10G10R10_UNORM_PACK32: (np.uint32, 1), capi.FORMAT_B10G11R11_UFLOAT_PACK32: (np.uint32, 1),
}


def layout_geometry(width, height, texel, layout):
    """(offset of the first texel in the allocation, pitch, bytes of the allocation)."""
    row = width * texel
    if layout == "tight":
        first, pitch = GUARD, row
    elif layout == "wide256":
        first, pitch = GUARD, (row + 255) // 256 * 256 + 256
    elif layout == "pad1":
        first, pitch = GUARD, row + texel
    elif layout == "off1":
        first, pitch = GUARD + texel, row + 3 * texel
    else:
        raise ValueError(f"unknown layout {layout!r}")
    return first, pitch, first + pitch * height + GUARD


class LayoutImage:
    def __init__(self, ctx, width, height, fmt, layout, fill=INPUT_FILL, buffer=None):
        self.ctx, self.layout, self.fill = ctx, layout, fill
        self.width, self.height, self.format = int(width), int(height), int(fmt)
        self.bpp = capi.FORMAT_BPP[fmt]
        self.first, self.pitch, self.nbytes = layout_geometry(self.width, self.height, self.bpp, layout)
        self.buffer = buffer if buffer is not None else capi.DeviceBuffer(ctx, self.nbytes)
        assert self.buffer.ptr % 256 == 0, "the layouts are stated relative to a 256-byte-aligned allocation"
        self.ptr = self.buffer.ptr + self.first
        self.desc = capi.Image(self.ptr, self.width, self.height, self.pitch, self.format)
        # what the allocation holds as far as the host knows: the fill, then whatever upload() wrote
        self.expected = np.full(self.nbytes, fill, np.uint8)
        self.buffer.upload(self.expected)

    def _rows(self, flat):
        """The texel bytes of every row as a (height, width * bpp) view of a whole-allocation byte array."""
        body = flat[self.first:self.first + self.pitch * self.height].reshape(self.height, self.pitch)
        return body[:, :self.width * self.bpp]

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.width * self.bpp * self.height, (a.shape, a.dtype, self.width, self.height, self.bpp)
        self._rows(self.expected)[:] = a.view(np.uint8).reshape(self.height, self.width * self.bpp)
        self.buffer.upload(self.expected)
        return self

    def download(self):
        tight = np.ascontiguousarray(self._rows(self.buffer.download(np.uint8)))
        if self.format not in _TEXEL:
            return tight
        dtype, components = _TEXEL[self.format]
        out = tight.view(dtype)
        return out.reshape(self.height, self.width, components) if components > 1 else out.reshape(self.height, self.width)

    def _region(self, offset):
        if offset < self.first:
            return "front guard"
        row, column = divmod(offset - self.first, self.pitch)
        if row >= self.height or (row == self.height - 1 and column >= self.width * self.bpp):
            return "back guard"
        if column >= self.width * self.bpp:
            return f"between rows (after row {row})"
        return f"texels (row {row}, x {column // self.bpp})"

    def _first_difference(self, got, texels_too, what):
        differs = got != self.expected
        if not texels_too:
            self._rows(differs)[:] = False
        if differs.any():
            offset = int(np.flatnonzero(differs)[0])
            raise AssertionError(f"{what} [{self.layout}, {self.width} x {self.height}, pitch {self.pitch}]: {self._region(offset)} touched, first at byte "
                                 f"{offset} of the allocation ({offset - self.first} from the first texel): {int(got[offset]):#04x}, was "
                                 f"{int(self.expected[offset]):#04x}; {int(differs.sum())} bytes in all")

    def check_guards(self, what="image"):
        """Every byte outside [row start, row start + width * texel) of every row still holds its fill."""
        self._first_difference(self.buffer.download(np.uint8), False, what)

    def check_unchanged(self, what="input"):
        """check_guards, and the texels are the uploaded ones."""
        self._first_difference(self.buffer.download(np.uint8), True, what)


class Factory:
    """make(width, height, format, role) -> LayoutImage, the layout chosen by role: 'in' (pure input), 'out' (written only), 'rmw'
    (read and written).  Keeps every image it made, so a test checks them all after the launches."""
    ASSIGNMENTS = {
        "tight": dict.fromkeys(("in", "out", "rmw"), "tight"),
        "wide256": dict.fromkeys(("in", "out", "rmw"), "wide256"),
        "pad1": dict.fromkeys(("in", "out", "rmw"), "pad1"),
        "mixed": {"in": "off1", "out": "pad1", "rmw": "off1"},
    }

    def __init__(self, ctx, assignment):
        self.ctx, self.assignment, self.by_role = ctx, assignment, self.ASSIGNMENTS[assignment]
        self.made = []  # (name, role, image)

    def __call__(self, width, height, fmt, role="in", name="", layout=None):
        image = LayoutImage(self.ctx, width, height, fmt, layout or self.by_role[role], OUTPUT_FILL if role == "out" else INPUT_FILL)
        self.made.append((name or f"image{len(self.made)}", role, image))
        return image

    def check(self):
        """check_unchanged() on every pure input, check_guards() on every other image."""
        for name, role, image in self.made:
            if role == "in":
                image.check_unchanged(name)
            else:
                image.check_guards(name)
