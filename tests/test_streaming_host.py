"""CPU: the host side of the stream ingest — phx_ingest_dims' arithmetic (streaming.py:59-62:
int(h * (set_width / w)), a truncated float64 product), the argument checks of phx_ingest that run
before anything is launched, and streaming.Stream over a directory and its refusals.  No GPU call is made."""
import os

import numpy as np
import pytest

from mladversarialobjectdetection_amd import _lib
from mladversarialobjectdetection_amd.streaming import Stream, ingest_dims

# (h, w), set_width, int(h * (set_width / w)), the exact floor h * set_width // w it is not
TRUNCATION = [((77, 77), 640, 639, 640), ((117, 78), 640, 959, 960), ((49, 49), 8, 7, 8), ((55, 11), 3, 14, 15)]


@pytest.mark.parametrize("hw,sw,want,floor", TRUNCATION)
def test_ingest_dims_truncates_the_float64_product(hw, sw, want, floor):
    h, w = hw
    assert int(h * (sw / w)) == want and h * sw // w == floor  # the case is what the issue says it is
    assert ingest_dims(sw, [hw]).tolist() == [[want, sw]]


def test_ingest_dims_batch_and_no_rescaling():
    dims = [(24, 40), (25, 40), (37, 53), (1080, 1920), (360, 640)]
    got = ingest_dims(20, dims)
    assert got.dtype == np.int32
    assert got.tolist() == [[int(h * (20 / w)), 20] for h, w in dims]
    assert got[:2].tolist() == [[12, 20], [12, 20]]
    assert ingest_dims(0, dims).tolist() == [list(d) for d in dims]
    assert ingest_dims(640, [(1080, 1920)]).tolist() == [[360, 640]]
    assert ingest_dims(1280, [(360, 640)]).tolist() == [[720, 1280]]


def _dims_rc(set_width, dims, B, out=True):
    lib = _lib.load()
    d = np.ascontiguousarray(np.asarray(dims if dims is not None else [(1, 1)], np.int32).reshape(-1, 2))
    o = np.full_like(d, -7)
    rc = lib.phx_ingest_dims(set_width, d.ctypes.data if dims is not None else None, B,
                             o.ctypes.data if out else None)
    return rc, lib.phx_last_error(None).decode(), o


def test_ingest_dims_refusals():
    rc, msg, o = _dims_rc(20, [(1, 100)], 1)
    assert rc == -1 and "dims[0] = 1x100" in msg and "is 0" in msg
    assert (o == -7).all()
    with pytest.raises(_lib.PhxError, match=r"dims\[1\] = 1x100"):
        ingest_dims(20, [(5, 5), (1, 100)])
    rc, msg, _ = _dims_rc(20, None, 1)
    assert rc == -1 and msg == "ingest_dims: dims is null"
    rc, msg, _ = _dims_rc(20, [(4, 4)], 1, out=False)
    assert rc == -1 and msg == "ingest_dims: out_dims is null"
    rc, msg, _ = _dims_rc(20, [(4, 4)], 0)
    assert rc == -1 and msg == "ingest_dims: B = 0 must be >= 1"
    rc, msg, _ = _dims_rc(-3, [(4, 4)], 1)
    assert rc == -1 and msg == "ingest_dims: set_width = -3 is negative"
    for bad in ((0, 4), (4, 0), (-1, 4)):
        rc, msg, _ = _dims_rc(20, [bad], 1)
        assert rc == -1 and "h and w must be >= 1" in msg
    rc, msg, _ = _dims_rc(2 ** 31 - 1, [(2 ** 31 - 1, 1)], 1)
    assert rc == -1 and "exceeds the int range" in msg


def test_ingest_checks_run_on_the_host():
    """every refusal of phx_ingest comes before any device call: a context on a machine without a GPU
    refuses with the argument's name (the pointers are never dereferenced)"""
    c = _lib.Context("efficientdet-d0", image_size=128, max_batch=2)
    lib = c.lib
    SRC, OUT = 1 << 20, 1 << 24  # stand-ins for device addresses
    off = np.zeros(3, np.int64)
    off[1:] = [4 * 4 * 3, 2 * 4 * 4 * 3]
    dims = np.asarray([[4, 4]] * 3, np.int32)
    oo = np.asarray([0, 2 * 2 * 3, 2 * 2 * 2 * 3], np.int64)

    def call(src=SRC, offsets=off, d=dims, B=2, sw=2, flags=0, out=OUT, out_offsets=oo):
        ptr = lambda a: a.ctypes.data if a is not None else None
        rc = lib.phx_ingest(c.h, src, ptr(offsets), ptr(d), B, sw, flags, out, ptr(out_offsets), None)
        return rc, lib.phx_last_error(c.h).decode()

    assert call(B=0) == (-1, "ingest: B = 0 must be >= 1")
    assert call(B=3) == (-4, "ingest: B = 3 exceeds max_batch = 2")
    assert call(src=None) == (-1, "ingest: src is null")
    assert call(offsets=None) == (-1, "ingest: offsets is null")
    assert call(d=None) == (-1, "ingest: dims is null")
    assert call(out=None) == (-1, "ingest: out is null")
    assert call(out_offsets=None) == (-1, "ingest: out_offsets is null")
    assert call(sw=-1) == (-1, "ingest: set_width = -1 is negative")
    assert call(flags=2) == (-1, "ingest: flags = 2 has an unknown bit")
    assert call(flags=3)[0] == -1
    rc, msg = call(d=np.asarray([[4, 4], [1, 100]], np.int32))
    assert rc == -1 and "dims[1] = 1x100" in msg and "is 0" in msg
    assert call(offsets=np.asarray([0, -48], np.int64)) == (-1, "ingest: offsets[1] is negative")
    assert call(out_offsets=np.asarray([0, -12], np.int64)) == (-1, "ingest: out_offsets[1] is negative")
    # output frame 1 (12 bytes at 11) overlaps output frame 0 (12 bytes at 0) by one byte
    rc, msg = call(out_offsets=np.asarray([0, 11], np.int64))
    assert rc == -1 and "out_offsets[1]" in msg and "overlaps output frame 0" in msg
    # output frame 0 starts on the last byte of source frame 1 (src + 48 .. src + 96), and in place
    rc, msg = call(out=SRC, out_offsets=np.asarray([95, 200], np.int64))
    assert rc == -1 and "out_offsets[0]" in msg and "overlaps source frame 1" in msg
    rc, msg = call(out=SRC, out_offsets=np.asarray([200, 0], np.int64), sw=0)
    assert rc == -1 and "out_offsets[1]" in msg and "overlaps source frame 0" in msg


def _write_png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_stream_over_a_directory(tmp_path):
    rng = np.random.default_rng(3)
    f2 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    f10 = rng.integers(0, 256, (6, 4, 3), dtype=np.uint8)
    _write_png(tmp_path / "preview10.png", f10)
    _write_png(tmp_path / "preview2.png", f2)
    (tmp_path / "notes.txt").write_text("not a frame")
    key = lambda x: int(x[len('preview'):-len('.png')])  # the demos' sort key
    st = Stream(str(tmp_path), filter_func=lambda f: f.endswith(".png"), sort_func=key)
    assert st.files == ["preview2.png", "preview10.png"] and st.set_width == 640
    got = list(st.frames())
    assert len(got) == 2
    for g, want in zip(got, (f2, f10)):
        assert g.dtype == np.uint8 and g.shape == want.shape and g.tobytes() == want.tobytes()
    # without the filter the listing keeps notes.txt, as the reference's does
    assert sorted(Stream(tmp_path, set_width=0).files) == ["notes.txt", "preview10.png", "preview2.png"]


def test_stream_over_frames_and_refusals(tmp_path):
    clip = np.arange(2 * 3 * 4 * 3, dtype=np.uint8).reshape(2, 3, 4, 3)
    got = list(Stream(clip, set_width=8, bgr=True).frames())
    assert len(got) == 2 and all((a == b).all() for a, b in zip(got, clip))  # raw: no swap, no resize
    assert len(list(Stream(iter([clip[0], clip[1][:2]])).frames())) == 2
    with pytest.raises(ValueError, match="HxWx3 uint8"):
        list(Stream([clip[0].astype(np.float32)]).frames())
    video = tmp_path / "clip.mp4"
    video.write_bytes(b"\x00" * 16)
    with pytest.raises(NotImplementedError, match="video decode"):
        Stream(str(video))
    with pytest.raises(NotImplementedError, match="webcam"):
        Stream(None)
    with pytest.raises(FileNotFoundError):
        Stream(os.path.join(str(tmp_path), "missing"))
    with pytest.raises(ValueError, match="negative"):
        Stream(clip, set_width=-1)
