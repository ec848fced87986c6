"""CPU: the bookkeeping of tests/layout_images.py on numpy alone, over a fake buffer: each layout's pointer and pitch, the round trip, and
that a stray byte in each guard region and a changed input texel are reported, each in its region."""
import numpy as np
import pytest

from granite_amd import capi
from layout_images import GUARD, INPUT_FILL, LAYOUTS, OUTPUT_FILL, Factory, LayoutImage, layout_geometry

F16, RGBA8, R8, D32 = capi.FORMAT_R16G16B16A16_SFLOAT, capi.FORMAT_R8G8B8A8_UNORM, capi.FORMAT_R8_UNORM, capi.FORMAT_D32_SFLOAT
BASE = 0x7000_0000_0000  # a fake, 256-byte-aligned device address; never dereferenced


class FakeBuffer:
    def __init__(self, nbytes):
        self.ptr, self.nbytes, self.bytes = BASE, nbytes, np.zeros(nbytes, np.uint8)

    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array).view(np.uint8).ravel()
        self.bytes[offset:offset + a.size] = a
        return self

    def download(self, dtype=np.uint8):
        return self.bytes.copy().view(dtype)


def make(w, h, fmt, layout, fill=INPUT_FILL):
    nbytes = layout_geometry(w, h, capi.FORMAT_BPP[fmt], layout)[2]
    return LayoutImage(None, w, h, fmt, layout, fill, buffer=FakeBuffer(nbytes))


def texels(w, h, fmt, seed=1):
    rng = np.random.default_rng(seed)
    if fmt == F16:
        return rng.integers(0, 0x7bff, (h, w, 4)).astype(np.uint16)
    if fmt == RGBA8:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    if fmt == R8:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    return rng.random((h, w)).astype(np.float32)


@pytest.mark.parametrize("fmt", [F16, RGBA8, R8, D32])
def test_each_layout_has_the_stated_pointer_and_pitch(fmt):
    t, w, h = capi.FORMAT_BPP[fmt], 10, 3
    want = {"tight": (0, w * t), "wide256": (0, 512), "pad1": (0, w * t + t), "off1": (t, w * t + 3 * t)}
    for layout in LAYOUTS:
        img = make(w, h, fmt, layout)
        assert (img.ptr - BASE - GUARD, img.pitch) == want[layout], layout
        assert (img.desc.ptr, img.desc.width, img.desc.height, img.desc.pitch_bytes, img.desc.format) == (img.ptr, w, h, img.pitch, fmt)
        assert img.pitch % t == 0 and img.ptr % t == 0 and img.pitch >= w * t
        assert img.nbytes == img.ptr - BASE + img.pitch * h + GUARD == img.buffer.nbytes
    assert make(256, 2, fmt, "wide256").pitch == 256 * t + 256  # a row that is a multiple of 256 already still gets the pad
    assert make(64, 2, fmt, "pad1").pitch % 16 != 0 and make(64, 2, fmt, "off1").ptr % 16 != 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", [F16, RGBA8, R8, D32])
def test_round_trip_and_untouched_guards(layout, fmt):
    w, h = 13, 5
    a = texels(w, h, fmt)
    img = make(w, h, fmt, layout).upload(a)
    got = img.download()
    assert got.dtype == a.dtype and got.shape == a.shape
    np.testing.assert_array_equal(got, a)
    img.check_guards()
    img.check_unchanged()
    raw = img.buffer.bytes
    assert (raw[:img.first] == INPUT_FILL).all() and (raw[-GUARD:] == INPUT_FILL).all()
    assert int((raw != INPUT_FILL).sum()) <= a.nbytes  # nothing but texels was written
    out = make(w, h, fmt, layout, OUTPUT_FILL)
    assert (out.buffer.bytes == OUTPUT_FILL).all()
    out.check_guards()


def guard_offsets(img):
    """One byte of each guard region: {region name the report must hold: offset in the allocation}."""
    row = img.width * img.bpp
    places = {"front guard": img.first - 1, "back guard": img.first + img.pitch * (img.height - 1) + row}
    if img.pitch > row:
        places["between rows (after row 1)"] = img.first + img.pitch + row  # the first pad byte of row 1
        places["between rows (after row 0)"] = img.first + img.pitch - 1    # the last pad byte of row 0
    return places


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", [F16, R8])
def test_a_stray_byte_is_reported_in_its_region(layout, fmt):
    probe = make(13, 5, fmt, layout)
    places = guard_offsets(probe)
    assert ("between rows (after row 1)" in places) == (layout != "tight")
    for region, offset in places.items():
        for check in ("check_guards", "check_unchanged"):
            img = make(13, 5, fmt, layout, OUTPUT_FILL).upload(texels(13, 5, fmt))
            img.buffer.bytes[offset] ^= 0x01
            with pytest.raises(AssertionError) as e:
                getattr(img, check)("probe")
            assert region in str(e.value) and f"first at byte {offset} " in str(e.value) and "probe" in str(e.value), (region, str(e.value))
    # the last byte of the allocation, and the first
    for offset, region in ((0, "front guard"), (probe.nbytes - 1, "back guard")):
        img = make(13, 5, fmt, layout)
        img.buffer.bytes[offset] = 0
        with pytest.raises(AssertionError, match=region):
            img.check_guards()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_changed_input_texel_is_reported_by_check_unchanged_only(layout):
    img = make(13, 5, F16, layout).upload(texels(13, 5, F16))
    offset = img.first + 3 * img.pitch + 7 * 8 + 2  # row 3, x 7
    img.buffer.bytes[offset] ^= 0x80
    img.check_guards()  # texels are the kernel's to write
    with pytest.raises(AssertionError) as e:
        img.check_unchanged("albedo")
    assert "texels (row 3, x 7)" in str(e.value) and "albedo" in str(e.value) and f"first at byte {offset} " in str(e.value)
    # the first and the last texel byte
    for offset, where in ((img.first, "row 0, x 0"), (img.first + 4 * img.pitch + 13 * 8 - 1, "row 4, x 12")):
        img = make(13, 5, F16, layout).upload(texels(13, 5, F16))
        img.buffer.bytes[offset] ^= 0x01
        with pytest.raises(AssertionError, match=where):
            img.check_unchanged()


def test_factory_assigns_layouts_by_role_and_checks_each_image(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", lambda ctx, nbytes: FakeBuffer(nbytes))
    want = {"tight": ("tight", "tight", "tight"), "wide256": ("wide256",) * 3, "pad1": ("pad1",) * 3, "mixed": ("off1", "pad1", "off1")}
    for assignment, layouts in want.items():
        make_image = Factory(None, assignment)
        images = [make_image(8, 4, F16, role, name=role) for role in ("in", "out", "rmw")]
        assert tuple(i.layout for i in images) == layouts
        assert [i.fill for i in images] == [INPUT_FILL, OUTPUT_FILL, INPUT_FILL]
        assert make_image(8, 4, F16, "in", layout="pad1").layout == "pad1"
        make_image.check()
        images[1].buffer.bytes[images[1].first] = 0  # an output's texel: its to write
        images[2].buffer.bytes[images[2].first] = 0
        make_image.check()
        images[0].buffer.bytes[images[0].first] = 0  # an input's texel
        with pytest.raises(AssertionError, match="in .*texels"):
            make_image.check()
        images[0].buffer.bytes[images[0].first] = INPUT_FILL
        images[1].buffer.bytes[0] = 0
        with pytest.raises(AssertionError, match="out .*front guard"):
            make_image.check()
