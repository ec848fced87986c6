"""CPU: the host-only part of Granite::Ocean (granite_amd/csrc/host/ocean_distribution.cpp) through the stand-alone tests/cpp/ocean_host.cpp,
built plainly and once with -fsanitize=address,undefined (host code with its own main; nothing is preloaded).

The Phillips distributions are held to float64: the program prints the raw draws of the same std:: engine and distribution in the same
order, and each entry must be that draw times a float64 amplitude * sqrt(phillips / 2) within 1e-4 relative plus 1e-6 of the array's
largest magnitude.  The bound is derived: the chain is about ten fp32 operations, and its worst conditioning is exp(-1 / (kL)^2) at the
lowest bin, where an argument near 100 turns 1e-7 relative into 1e-5; the absolute term covers fp32 denormals."""
import os

import numpy as np
import pytest

from host_program import ROOT, program_fixtures, run_program

plain, sanitized = program_fixtures(["ocean_host.cpp", os.path.join(ROOT, "granite_amd", "csrc", "host", "ocean_distribution.cpp")])
# fft_resolution, displacement_downsample, grid_count, grid_resolution, ocean_size, wind, heightmap
CONFIGS = {"small": (128, 1, 4, 32, 128.0, (4.0, 2.0), 1), "default_grid": (128, 1, 64, 128, 1024.0, (4.0, 2.0), 1),
           "plane": (64, 0, 64, 128, 1024.0, (-3.0, 0.5), 0)}
NORMAL_MOD, AMPLITUDE, G = 7.3, 0.2, 9.81


def run_dist(exe, config):
    n, shift, count, resolution, size, wind, heightmap = config
    raw = run_program(exe, "dist", n, shift, count, resolution, repr(size), repr(wind[0]), repr(wind[1]), heightmap)
    data = np.frombuffer(raw, np.float32)
    m = n >> shift
    assert data.size == 8 + 2 * (n * n + m * m + n * n)
    header, rest = data[:8], data[8:]
    return header, rest[:2 * n * n].reshape(n, n, 2), rest[2 * n * n:2 * (n * n + m * m)].reshape(m, m, 2), rest[2 * (n * n + m * m):].reshape(n, n, 2)


def expected(draws, n, world, amplitude, wind):
    """float64: draw * amplitude * sqrt(0.5 * phillips(k)), k = 2 pi / world * alias(i)"""
    wind = np.asarray(wind, np.float64)
    speed2 = float(wind @ wind)
    direction, big_l = wind / np.sqrt(speed2), speed2 / G
    index = np.arange(n)
    f = np.where(index > n // 2, index - n, index).astype(np.float64)
    kx, ky = np.meshgrid(2.0 * np.pi / world * f, 2.0 * np.pi / world * f)  # rows are z
    k = np.hypot(kx, ky)
    with np.errstate(divide="ignore", invalid="ignore"):
        kw = (kx * direction[0] + ky * direction[1]) / k
        p = kw * kw * np.exp(-k * k * 0.02 * 0.02) * np.exp(-1.0 / (k * big_l) ** 2) * k ** -4.0
    p[0, 0] = 0.0
    return draws.reshape(n, n, 2).astype(np.float64) * (amplitude * np.sqrt(0.5 * p))[..., None]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_distributions(plain, name):
    config = CONFIGS[name]
    n, shift, count, resolution, size, wind, _ = config
    header, height, disp, normal = run_dist(plain, config)
    world = size / count * n / resolution
    amplitude = AMPLITUDE * np.sqrt(1.0 / world ** 2)
    assert np.allclose(header[:4], [world, world, world / NORMAL_MOD, world / NORMAL_MOD], rtol=1e-6)
    assert np.allclose(header[4:6], np.asarray(wind) / np.hypot(*wind), rtol=1e-6) and np.isclose(header[6], (wind[0] ** 2 + wind[1] ** 2) / G, rtol=1e-6)
    assert np.isclose(header[7], amplitude, rtol=1e-6)
    draws = np.frombuffer(run_program(plain, "draws", 2 * n * n), np.float32)
    for got, w, a in ((height, world, amplitude), (normal, world / NORMAL_MOD, amplitude * NORMAL_MOD)):
        want = expected(draws, n, w, a, wind)
        error = np.abs(got.astype(np.float64) - want)
        bound = 1e-4 * np.abs(want) + 1e-6 * np.abs(want).max()
        print(f"{name}: largest error / bound {np.max(error / bound):.3g}")
        assert np.all(error <= bound)
        assert got[0, 0, 0] == 0.0 and got[0, 0, 1] == 0.0  # the DC bin
    # an exact gather: bin i of the small spectrum is bin alias(i) of the large one, negative frequencies from its end
    m = n >> shift
    index = np.arange(m)
    index = np.where(index > m // 2, index - m + n, index)
    assert np.array_equal(disp, height[index][:, index])
    # the same draws: the normal distribution differs from the height one only by mod and amplitude
    assert not np.array_equal(normal, height)
    both = (height[..., 0] != 0) & (normal[..., 0] != 0)
    assert both.sum() > n * n // 4
    assert np.allclose(height[..., 1][both] / height[..., 0][both], normal[..., 1][both] / normal[..., 0][both], rtol=1e-5)


def test_refusals(plain):
    run_program(plain, "refusals")


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, plain):
    run_program(sanitized, "refusals")
    for name in ("small", "plane"):
        a, b = run_dist(sanitized, CONFIGS[name]), run_dist(plain, CONFIGS[name])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
