"""GPU: phx_ingest (streaming.Stream.change_frame_size on the device, csrc/kernels_ingest.hip) against
oracle.adv_patch.resize_linear_u8 — exact uint8 equality, no tolerance — on seeded random frames.

Every raw call runs between guard bytes: in front of the output buffer, between the frames and behind the
last one, which must come back unchanged.  Each shape runs twice: with 4-byte aligned source and output
offsets (the dword stores, and the box mode's dword loads) and with odd ones (the byte paths)."""
import numpy as np
import pytest
import torch

from oracle.adv_patch import resize_linear_u8

pytestmark = pytest.mark.gpu

GUARD = 0xA5
MAX_BATCH = 4

# (h, w), set_width, the result's size where the issue states it
SHAPES = [((37, 53), 20, (13, 20)),     # fractional downscale
          ((23, 31), 80, (59, 80)),     # upscale: sx < 0, sx >= W - 1, ys = -1 and ys + 1 = H clamps
          ((24, 40), 20, (12, 20)),     # 2x box
          ((25, 40), 20, (12, 20)),     # x factor 2 but linear
          ((9, 20), 20, (9, 20)),       # copy
          ((1, 8), 16, (2, 16)),        # one source row
          ((5, 1), 4, (20, 4)),         # one source column
          ((3, 2), 5, (7, 5)),          # two source columns: the smallest frame of the 6-byte tap loads
          ((2, 3), 7, (4, 7)),          # odd row pitch: byte stores
          ((77, 77), 640, (639, 640)),  # truncated height
          ((180, 320), 640, (360, 640))]  # one realistic frame


@pytest.fixture(scope="module")
def ctx():
    from mladversarialobjectdetection_amd import _lib
    return _lib.Context("efficientdet-d0", image_size=128, max_batch=MAX_BATCH)


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _want(frame, set_width, bgr=False):
    h, w, _ = frame.shape
    if bgr:
        frame = np.ascontiguousarray(frame[..., ::-1])
    if not set_width:
        return frame.copy()
    return resize_linear_u8(frame, set_width, int(h * (set_width / w)))


def _layout(sizes, lead, gaps):
    """byte offsets of items of `sizes` after `lead` bytes, item i followed by gaps[i] bytes -> (offsets, total)"""
    off, pos = [], lead
    for n, g in zip(sizes, gaps):
        off.append(pos)
        pos += n + g
    return np.asarray(off, np.int64), pos


def _raw(ctx, frames, set_width, *, flags=0, src_lead=16, out_lead=16, gaps=None, expect_rc=0):
    """one phx_ingest over `frames` packed with guard bytes around every source and output frame ->
    (list of output frames, return code); asserts that no guard byte of the output changed"""
    from mladversarialobjectdetection_amd.attacker import _stream
    B = len(frames)
    gaps = gaps or [8] * B
    dims = np.asarray([f.shape[:2] for f in frames], np.int32)
    # (a refused negative set_width gets an output buffer of the sources' size: all guard bytes)
    odims = np.asarray([(int(h * (set_width / w)), set_width) if set_width > 0 else (h, w) for h, w in dims], np.int32)
    soff, stotal = _layout([f.size for f in frames], src_lead, gaps)
    osz = [int(h) * int(w) * 3 for h, w in odims]
    ooff, ototal = _layout(osz, out_lead, gaps)
    src = np.full(stotal, GUARD, np.uint8)
    for f, o in zip(frames, soff):
        src[o:o + f.size] = f.reshape(-1)
    dsrc = torch.as_tensor(src).cuda()
    dout = torch.full((ototal,), GUARD, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.phx_ingest(ctx.h, dsrc.data_ptr(), soff.ctypes.data, dims.ctypes.data, B, set_width, flags,
                            dout.data_ptr(), ooff.ctypes.data, _stream())
    assert rc == expect_rc, ctx.lib.phx_last_error(ctx.h)
    out = dout.cpu().numpy()
    assert (dsrc.cpu().numpy() == src).all()
    outside = np.ones(ototal, bool)
    got = []
    for o, n, (h, w) in zip(ooff, osz, odims):
        outside[o:o + n] = False
        got.append(out[o:o + n].reshape(h, w, 3))
    assert (out[outside] == GUARD).all(), "a byte outside the frames was written"
    if rc != 0:
        assert (out == GUARD).all(), "a refused call wrote"
    return got, rc


@pytest.mark.parametrize("lead", [(16, 16), (3, 5)], ids=["aligned", "odd"])
@pytest.mark.parametrize("hw,set_width,size", SHAPES, ids=[f"{h}x{w}to{s}" for (h, w), s, _ in SHAPES])
def test_ingest_equals_the_oracle(ctx, hw, set_width, size, lead):
    fr = _frame(*hw, seed=hw[0] * 1000 + hw[1])
    want = _want(fr, set_width)
    assert want.shape[:2] == size
    got, _ = _raw(ctx, [fr], set_width, src_lead=lead[0], out_lead=lead[1])
    np.testing.assert_array_equal(got[0], want)


def test_three_modes_in_one_batch_at_odd_offsets(ctx):
    """box, linear and copy frames in one launch; odd gaps put every frame at another alignment"""
    frames = [_frame(24, 40, 1), _frame(25, 40, 2), _frame(12, 20, 3), _frame(37, 53, 4)]
    for lead, gaps in (((1, 3), [1, 2, 3, 5]), ((16, 16), [8, 8, 8, 8]), ((2, 1), [7, 1, 6, 3])):
        got, _ = _raw(ctx, frames, 20, src_lead=lead[0], out_lead=lead[1], gaps=gaps)
        for g, f in zip(got, frames):
            np.testing.assert_array_equal(g, _want(f, 20))


@pytest.mark.parametrize("hw,set_width", [((37, 53), 20), ((24, 40), 20), ((9, 20), 20), ((11, 13), 0)])
def test_bgr_reads_the_channels_reversed(ctx, hw, set_width):
    from mladversarialobjectdetection_amd import _lib
    fr = _frame(*hw, seed=9)
    for lead in ((16, 16), (1, 3)):
        got, _ = _raw(ctx, [fr], set_width, flags=_lib.INGEST_BGR, src_lead=lead[0], out_lead=lead[1])
        np.testing.assert_array_equal(got[0], _want(fr, set_width, bgr=True))


def test_set_width_zero_copies(ctx):
    frames = [_frame(7, 9, 5), _frame(3, 4, 6)]
    got, _ = _raw(ctx, frames, 0, src_lead=3, out_lead=1, gaps=[5, 2])
    for g, f in zip(got, frames):
        np.testing.assert_array_equal(g, f)


def test_refusals_launch_nothing(ctx):
    """the checks of include/phx.h with real device buffers: the output stays untouched"""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.attacker import _stream
    lib = ctx.lib
    fr = [_frame(8, 8, 1), _frame(8, 8, 2)]
    err = lambda: lib.phx_last_error(ctx.h).decode()
    _raw(ctx, fr, 4, flags=2, expect_rc=-1)
    assert "unknown bit" in err()
    _raw(ctx, fr, -4, expect_rc=-1)
    assert "set_width = -4 is negative" in err()
    _raw(ctx, [_frame(1, 100, 3)], 20, expect_rc=-1)
    assert "dims[0] = 1x100" in err() and "is 0" in err()
    _raw(ctx, [_frame(4, 4, i) for i in range(MAX_BATCH + 1)], 2, expect_rc=-4)
    assert f"B = {MAX_BATCH + 1} exceeds max_batch = {MAX_BATCH}" in err()
    # overlap: hand-made tables over one buffer that holds both the sources and the outputs
    buf = torch.full((1024,), GUARD, dtype=torch.uint8, device="cuda")
    dims = np.asarray([[8, 8], [8, 8]], np.int32)
    soff = np.asarray([0, 192], np.int64)

    def call(out_ptr, ooff, B=2):
        ooff = np.asarray(ooff, np.int64)
        rc = lib.phx_ingest(ctx.h, buf.data_ptr(), soff.ctypes.data, dims.ctypes.data, B, 4, 0, out_ptr,
                            ooff.ctypes.data, _stream())
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == GUARD).all()
        return rc, err()

    rc, msg = call(buf.data_ptr(), [383, 600])  # the last byte of source frame 1
    assert rc == -1 and "out_offsets[0]" in msg and "overlaps source frame 1" in msg
    rc, msg = call(buf.data_ptr(), [400, 447])  # 48-byte outputs one byte into each other
    assert rc == -1 and "out_offsets[1]" in msg and "overlaps output frame 0" in msg
    rc, msg = call(buf.data_ptr() + 384, [-1, 100])
    assert rc == -1 and "out_offsets[0] is negative" in msg
    rc, msg = call(None, [400, 500])
    assert rc == -1 and "out is null" in msg
    rc, msg = call(buf.data_ptr() + 384, [0, 48], B=0)
    assert rc == -1 and "B = 0" in msg
    # the neighbouring call is accepted: the outputs directly behind the sources, touching them
    ooff = np.asarray([0, 48], np.int64)
    rc = lib.phx_ingest(ctx.h, buf.data_ptr(), soff.ctypes.data, dims.ctypes.data, 2, 4, 0, buf.data_ptr() + 384,
                        ooff.ctypes.data, _stream())
    assert rc == 0, err()
    out = buf.cpu().numpy()
    assert (out[:384] == GUARD).all() and (out[480:] == GUARD).all()
    box = np.full((4, 4, 3), GUARD, np.uint8)  # the 2x2 box mean of a constant frame
    assert (out[384:480] == np.concatenate([box.reshape(-1)] * 2)).all()


def test_stream_methods_agree_with_the_raw_call(ctx):
    from mladversarialobjectdetection_amd.detector import PackedFrames
    from mladversarialobjectdetection_amd.streaming import Stream, unpack_device
    frames = [_frame(37, 53, 11), _frame(24, 40, 12), _frame(12, 20, 13), _frame(25, 40, 14), _frame(23, 31, 15),
              _frame(5, 1, 16)]
    want, _ = _raw(ctx, frames[:4], 20)
    want += _raw(ctx, frames[4:], 20)[0]
    st = Stream(frames, set_width=20, ctx=ctx)
    p = st.change_frame_size(frames)  # six frames, max_batch 4: two launches into one buffer
    assert isinstance(p, PackedFrames) and p.dims.tolist() == [list(w.shape[:2]) for w in want]
    assert p.offsets.tolist() == np.concatenate([[0], np.cumsum([w.size for w in want])[:-1]]).tolist()
    for g, w in zip(unpack_device(p), want):
        assert g.is_cuda and g.dtype == torch.uint8
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    one = st.change_frame_size(frames[0])
    np.testing.assert_array_equal(unpack_device(one)[0].cpu().numpy(), want[0])
    batches = list(st.batches(4))
    assert [len(b.offsets) for b in batches] == [4, 2]
    flat = [g for b in batches for g in unpack_device(b)]
    played = list(Stream(iter(frames), set_width=20, ctx=ctx).play())
    assert len(flat) == len(played) == 6
    for g, q, w in zip(flat, played, want):
        assert tuple(q.shape) == w.shape
        np.testing.assert_array_equal(g.cpu().numpy(), w)
        np.testing.assert_array_equal(q.cpu().numpy(), w)
    # a batch array and the BGR flag
    clip = np.stack([_frame(10, 14, 20), _frame(10, 14, 21)])
    got = unpack_device(Stream(clip, set_width=7, bgr=True, ctx=ctx).change_frame_size(clip))
    for g, f in zip(got, clip):
        np.testing.assert_array_equal(g.cpu().numpy(), _want(f, 7, bgr=True))
