"""CPU: the three push blocks of the ocean entry points have the shaders' layout in the ctypes binding (the header asserts the same in C)."""
import ctypes as C

from granite_amd import capi


def test_push_block_sizes_and_offsets():
    g, b, m = capi.PushOceanGenerate, capi.PushOceanBake, capi.PushOceanMipmap
    assert C.sizeof(g) == 28
    assert (g.mod_factor.offset, g.N.offset, g.freq_to_band_mod.offset, g.time.offset, g.period.offset) == (0, 8, 16, 20, 24)
    assert C.sizeof(b) == 32
    assert (b.inv_size.offset, b.scale.offset) == (0, 16)
    assert C.sizeof(m) == 36
    assert (m.result_mod.offset, m.inv_resolution.offset, m.count.offset, m.lod.offset) == (0, 16, 24, 32)


def test_entry_points_are_bound():
    lib = capi.load_library()
    for name in ("gr_ocean_generate_fft", "gr_ocean_bake_maps", "gr_ocean_mipmap"):
        assert name in capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
