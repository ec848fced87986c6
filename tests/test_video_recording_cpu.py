"""CPU: the recording side that needs no device: the headless runner's --video-encode-path writers (YUV4MPEG2 / raw), its command line,
the packed-frame split of granite_amd.app, and the recorder's refusal of row bands."""
import numpy as np
import pytest

from granite_amd import app as gapp
from granite_amd import capi, headless


def synthetic_frames(w, h, fmt):
    wide = fmt.endswith("16") or fmt in ("p010", "p016")
    sub = "444" not in fmt
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    dt = np.uint16 if wide else np.uint8
    frames = []
    for k in range(2):
        y = (np.arange(w * h) * 7 + k).astype(dt).reshape(h, w)
        cb = np.full((ch, cw), 100 + k, dt)
        cr = np.full((ch, cw), 200 + k, dt)
        frames.append((y, cb, cr))
    return frames


@pytest.mark.parametrize("fmt,tag", [("yuv420p", b"C420jpeg"), ("yuv444p", b"C444"), ("yuv420p16", b"C420p16"), ("yuv444p16", b"C444p16")])
def test_y4m_writer_header_and_plane_order(tmp_path, fmt, tag):
    w, h = 6, 4
    path = str(tmp_path / "a.y4m")
    wr = headless.VideoWriter(path, w, h, 1.0 / 60.0, fmt)
    frames = synthetic_frames(w, h, fmt)
    for y, cb, cr in frames:
        wr.write(np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).view(np.uint8))
    wr.close()
    data = open(path, "rb").read()
    header, _, body = data.partition(b"\n")
    fields = header.split()
    assert fields[:4] == [b"YUV4MPEG2", b"W6", b"H4", b"F60:1"]
    assert tag in fields and b"XCOLORRANGE=FULL" in fields
    parts = body.split(b"FRAME\n")
    assert parts[0] == b"" and len(parts) == 3
    for (y, cb, cr), raw in zip(frames, parts[1:]):
        a = np.frombuffer(raw, y.dtype)
        n, c = y.size, cb.size
        np.testing.assert_array_equal(a[:n].reshape(y.shape), y)       # Y, then Cb, then Cr
        np.testing.assert_array_equal(a[n:n + c].reshape(cb.shape), cb)
        np.testing.assert_array_equal(a[n + c:].reshape(cr.shape), cr)


@pytest.mark.parametrize("hdr10", [False, True])
def test_raw_writer_is_concatenated_nv12_or_p010(tmp_path, hdr10):
    path = str(tmp_path / "a.yuv")
    fmt = headless.VideoWriter.format_for(path, hdr10)
    assert fmt == ("p010" if hdr10 else "nv12")
    assert headless.VideoWriter.format_for(str(tmp_path / "a.Y4M"), hdr10) == ("yuv420p16" if hdr10 else "yuv420p")
    w, h = 4, 2
    dt = np.uint16 if hdr10 else np.uint8
    frames = [np.arange(w * h * 3 // 2, dtype=dt) + k for k in range(2)]
    wr = headless.VideoWriter(path, w, h, 0.01, fmt)
    for f in frames:
        wr.write(f.view(np.uint8))
    wr.close()
    np.testing.assert_array_equal(np.fromfile(path, dt), np.concatenate(frames))


def test_video_encode_path_parses_without_a_device():
    args = headless.parse_args(["synthetic", "--frames", "3", "--video-encode-path", "out.y4m"])
    assert args.video_encode_path == "out.y4m" and args.frames == 3
    assert headless.parse_args(["synthetic", "--frames", "1"]).video_encode_path == ""


def test_packed_frame_split():
    layout = gapp.VideoLayout()
    layout.num_planes, layout.bytes_per_sample = 2, 2
    layout.width[:] = [5, 3, 0]
    layout.height[:] = [3, 2, 0]
    layout.pitch[:] = [10, 12, 0]
    layout.offset[:] = [0, 30, 0]
    layout.frame_bytes = 54
    buf = np.arange(27, dtype=np.uint16).view(np.uint8)
    y, uv = gapp.video_planes(layout, buf)
    assert y.shape == (3, 5) and uv.shape == (2, 3, 2)
    assert y[2, 4] == 14 and tuple(uv[1, 2]) == (25, 26)


def test_recording_refuses_row_bands():
    a = gapp.Application(320, 180, device=-1, strip_index=0, strip_count=2)
    with pytest.raises(capi.GraniteHipError, match="row bands"):
        a.start_video("nv12")
    a.close()


def test_recording_symbols_are_bound():
    lib = gapp.load_library()
    for name in ("gra_video_begin", "gra_video_frame_layout", "gra_video_read_frame", "gra_video_end"):
        assert name in gapp.EXPORTED_SYMBOLS and hasattr(lib, name)
