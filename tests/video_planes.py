"""What the video tests share: plane layouts as [(w, h, format), ...], the edge sizes of the 4 x 2-pixel-per-lane kernels, and an image
placed inside a guarded device allocation."""
import numpy as np

from granite_amd import capi

R8, R16, R8G8, R16G16 = capi.FORMAT_R8_UNORM, capi.FORMAT_R16_UNORM, capi.FORMAT_R8G8_UNORM, capi.FORMAT_R16G16_UNORM

GUARD = 4096
FILL = 0xA5
# k_video_direct and k_yuv_to_rgb convert 4 x 2 pixels per lane, 256 pixels per group row and 8 rows per group
EDGE_SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 3), (7, 9), (255, 1), (256, 2), (257, 3), (1023, 7)]
# samples per texel and their type, of the formats whose rows samples() views
CHANNELS = {R8: (1, np.uint8), R16: (1, np.uint16), R8G8: (2, np.uint8), R16G16: (2, np.uint16),
            capi.FORMAT_R8G8B8A8_UNORM: (4, np.uint8), capi.FORMAT_B8G8R8A8_UNORM: (4, np.uint8),
            capi.FORMAT_R8G8B8A8_SRGB: (4, np.uint8), capi.FORMAT_B8G8R8A8_SRGB: (4, np.uint8)}


def nv12(w, h, wide=False):
    return [(w, h, R16 if wide else R8), ((w + 1) // 2, (h + 1) // 2, R16G16 if wide else R8G8)]


def yuv(w, h, sub=True, wide=False):
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    f = R16 if wide else R8
    return [(w, h, f), (cw, ch, f), (cw, ch, f)]


class GuardedImage:
    """An image inside a larger allocation, `offset` bytes in, with a row pitch of row + pad bytes (by default padded to a multiple of
    16 plus 16: the vector loads / stores), GUARD bytes after the last row; everything outside the rows holds FILL.  data: what the rows
    hold (None: FILL, an output).  An offset or pitch that is not a multiple of 16 takes the element-by-element path."""

    def __init__(self, gr, w, h, fmt, data=None, offset=0, pad=None):
        self.w, self.h, self.fmt, self.offset = w, h, fmt, offset
        self.row = w * capi.FORMAT_BPP[fmt]
        self.pitch = (self.row + 15) // 16 * 16 + 16 if pad is None else self.row + pad
        self.buf = capi.DeviceBuffer(gr, offset + self.pitch * h + GUARD)
        raw = np.full(self.buf.nbytes, FILL, np.uint8)
        if data is not None:
            raw[offset:offset + self.pitch * h].reshape(h, self.pitch)[:, :self.row] = np.ascontiguousarray(data).view(np.uint8).reshape(h, self.row)
        self.buf.upload(raw)
        self.desc = capi.Image(self.buf.ptr + offset, w, h, self.pitch, fmt)

    def read(self):
        """The rows as bytes, (h, row); nothing outside them may have changed."""
        raw = self.buf.download(np.uint8)
        assert (raw[:self.offset] == FILL).all(), "bytes written before the image"
        raw = raw[self.offset:]
        rows = raw[:self.pitch * self.h].reshape(self.h, self.pitch)
        assert (rows[:, self.row:] == FILL).all(), "bytes written in a row's pitch padding"
        assert (raw[self.pitch * self.h:] == FILL).all(), "bytes written after the image's last row"
        return np.ascontiguousarray(rows[:, :self.row])

    def samples(self):
        """read() as samples: (h, w) or (h, w, channels)."""
        ch, dtype = CHANNELS[self.fmt]
        data = self.read().view(dtype)
        return data.reshape(self.h, self.w, ch) if ch > 1 else data.reshape(self.h, self.w)

    def untouched(self):
        return bool((self.buf.download(np.uint8) == FILL).all())
