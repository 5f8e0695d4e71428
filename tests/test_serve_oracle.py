"""CPU: hand-checkable pins of the serving restatement (tests/serve_oracle.py) and the serving entry
points' argument checks through the C ABI — every refusal is decided on the host, nothing is launched."""
import numpy as np
import pytest

import serve_oracle as so
from mladversarialobjectdetection_amd import _lib
from mladversarialobjectdetection_amd.attacker import MEAN_RGB, STDDEV_RGB

f32 = np.float32
MEAN, STD = MEAN_RGB["efficientdet"], STDDEV_RGB["efficientdet"]


def _norm(frame):
    return (frame.astype(np.float64) - np.asarray(MEAN, f32).astype(np.float64)) / np.asarray(STD, f32).astype(np.float64)


def test_dims_truncate_in_fp32():
    # 97 * fp32(128 / 97) = 127.99999 -> 127: column 127 of that canvas is padding
    assert so.dims(60, 97, 128)[:2] == (79, 127)
    sh, sw, s = so.dims(720, 1280, 640)
    assert (sh, sw) == (360, 640) and s == f32(0.5) and so.scale_to_original(720, 1280, 640) == f32(2.0)
    assert so.dims(96, 160, 128)[:2] == (76, 128)
    assert so.dims(128, 128, 128) == (128, 128, f32(1.0))


def test_identity_frame_is_the_normalised_frame():
    fr = np.random.default_rng(0).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    np.testing.assert_array_equal(so.preprocess64(fr, 16, MEAN, STD), _norm(fr))


def test_downscale_of_a_row_constant_frame():
    # constant along each row (the value depends on the column and channel only): a 2x vertical
    # average changes nothing, and the 2x horizontal one is the mean of each column pair.  The
    # normalised triangle weights of a 2x downscale are (1/8, 3/8, 3/8, 1/8) inside the frame.
    rng = np.random.default_rng(1)
    col = rng.integers(0, 256, (1, 32, 3), dtype=np.uint8)
    const = np.broadcast_to(col[:, :1], (32, 32, 3)).copy()     # one value per channel
    out = so.preprocess64(const, 16, MEAN, STD)
    np.testing.assert_allclose(out, np.broadcast_to(_norm(const)[:1, :1], (16, 16, 3)), rtol=0, atol=1e-6)
    fr = np.broadcast_to(col, (32, 32, 3)).copy()
    out = so.preprocess64(fr, 16, MEAN, STD)
    n = _norm(fr)[0]
    np.testing.assert_allclose(out, np.broadcast_to(out[:1], out.shape), rtol=0, atol=1e-6)  # rows equal
    want = (n[1:29:2] + 3 * n[2:30:2] + 3 * n[3:31:2] + n[4:32:2]) / 8                       # columns 1..14
    np.testing.assert_allclose(out[0, 1:15], want, rtol=0, atol=1e-6)


def test_pad_region_is_exactly_zero():
    fr = np.random.default_rng(2).integers(0, 256, (60, 97, 3), dtype=np.uint8)
    out = so.preprocess64(fr, 128, MEAN, STD)
    assert np.array_equal(out[79:], np.zeros_like(out[79:])) and np.array_equal(out[:, 127:], np.zeros_like(out[:, 127:]))
    assert out[:79, 126].any()
    assert np.abs(out[:79, :127]).max() <= 2.65  # the bound the GPU test's tolerance uses


def test_postprocess_global_hand_case():
    # four boxes in two classes at S = 100: A and B overlap (IoU 0.81), C is disjoint and sticks out of
    # the image, D is below the threshold.  NMS is global: B is decayed by A although their classes
    # differ.  Clip comes before the scale; classes are argmax + 1 as float32.
    boxes = np.array([[10, 10, 50, 50], [10, 10, 46, 46], [60, 60, 120, 90], [0, 0, 5, 5]], f32)
    scores = np.array([0.9, 0.8, 0.7, 0.4], f32)
    classes = np.array([0, 16, 16, 0])
    ob, os_, oc, n = so.postprocess_global(boxes, scores, classes, 100, 0.5, scale=f32(1.5))
    assert n == 2  # B: 0.8 * exp(-2 * 0.81^2) = 0.215 <= 0.5 drops out
    np.testing.assert_array_equal(ob[:2], np.array([[15, 15, 75, 75], [90, 90, 150, 135]], f32))  # 120 -> 100 -> 150
    np.testing.assert_array_equal(os_[:2], np.array([0.9, 0.7], f32))
    np.testing.assert_array_equal(oc[:2], np.array([1, 17], f32))
    assert not ob[2:].any() and not os_[2:].any() and not oc[2:].any()
    ob, os_, oc, n = so.postprocess_global(boxes, scores, classes, 100, 0.001)
    assert n == 4 and oc[:4].tolist() == [1, 17, 1, 17]  # A, C, D, then the decayed B
    iou = f32(36 * 36) / f32(40 * 40)
    np.testing.assert_allclose(os_[3], 0.8 * np.exp(-2.0 * float(iou) ** 2), rtol=1e-6)
    np.testing.assert_array_equal(ob[1], np.array([60, 60, 100, 90], f32))  # no scale: model pixels


# ---- argument checks through the ABI (no GPU work) ----------------------------------------------
def _tables(shapes):
    dims = np.asarray(shapes, np.int32).reshape(-1, 2)
    sizes = [int(h) * int(w) * 3 for h, w in dims]
    off = np.zeros(len(sizes), np.int64)
    off[1:] = np.cumsum(sizes)[:-1]
    return off, dims


def _refused(c, name, *args):
    rc = getattr(c.lib, name)(c.h, *args)
    return rc, c.lib.phx_last_error(c.h).decode()


@pytest.mark.parametrize("entry", ["phx_serve_preprocess", "phx_serve"])
def test_serve_errors_without_gpu_work(entry):
    c = _lib.Context("efficientdet-d0", image_size=128, max_batch=2)
    SRC = 4096  # stands for a device address: every case below is refused before it is read
    outs = (4096, 4096) if entry == "phx_serve_preprocess" else (4096, 4096, 4096, 4096, None)

    def call(src, shapes, B=None):
        off, dims = _tables(shapes)
        return _refused(c, entry, src, off.ctypes.data, dims.ctypes.data, len(shapes) if B is None else B, *outs, None)

    rc, msg = call(SRC, [(64, 64)], B=0)
    assert rc == -1 and "B = 0" in msg
    rc, msg = call(SRC, [(64, 64)] * 3)
    assert rc == -1 and "B = 3" in msg and "max_batch = 2" in msg
    rc, msg = call(None, [(64, 64)])
    assert rc == -1 and "src" in msg
    rc, msg = call(SRC, [(64, 64), (0, 5)])
    assert rc == -1 and "dims[1]" in msg and "0x5" in msg
    # int(fp32(1) * fp32(128 / 300)) = 0: tf.image.resize raises on an empty size
    rc, msg = call(SRC, [(1, 300)])
    assert rc == -1 and "dims[0]" in msg and "scaled height" in msg
    rc, msg = _refused(c, entry, SRC, None, None, 1, *outs, None)
    assert rc == -1 and "offsets" in msg


def test_serve_refuses_null_outputs_and_bf16_contexts():
    off, dims = _tables([(64, 64)])
    c = _lib.Context("efficientdet-d0", image_size=128, max_batch=2)
    rc, msg = _refused(c, "phx_serve_preprocess", 4096, off.ctypes.data, dims.ctypes.data, 1, None, 4096, None)
    assert rc == -1 and "images" in msg
    rc, msg = _refused(c, "phx_serve_preprocess", 4096, off.ctypes.data, dims.ctypes.data, 1, 4100, 4096, None)
    assert rc == -1 and "16-byte" in msg
    # good arguments, no weights: refused as a state error before any device call
    rc, msg = _refused(c, "phx_serve", 4096, off.ctypes.data, dims.ctypes.data, 1, 4096, 4096, 4096, 4096, None, None)
    assert rc == -3 and "weights not loaded" in msg
    rc, msg = _refused(c, "phx_nms_global", 4096, 4096, None, None, 1, 8, None, 4096, 4096, 4096, 4096, None)
    assert rc == -1 and "classes" in msg
    # phx.h: phx_serve runs in fp32 contexts only
    cb = _lib.Context("efficientdet-d0", image_size=128, max_batch=2, compute_dtype=_lib.DTYPE_BF16)
    rc, msg = _refused(cb, "phx_serve", 4096, off.ctypes.data, dims.ctypes.data, 1, 4096, 4096, 4096, 4096, None, None)
    assert rc == -1 and "BF16" in msg


def test_context_constants_are_the_reference_float32():
    # tf.constant(mean_rgb, dtype=tf.float32) of the Python doubles 0.485 * 255, ... (dataloader.py:63-64)
    for name, fam in (("efficientdet-d0", "efficientdet"), ("efficientdet-lite0", "lite")):
        info = _lib.Context(name, image_size=128, max_batch=1).model_info()
        assert [f32(v) for v in info["mean_rgb"]] == [f32(v) for v in MEAN_RGB[fam]]
        assert [f32(v) for v in info["stddev_rgb"]] == [f32(v) for v in STDDEV_RGB[fam]]


def test_detector_params_and_filter_by_thresh():
    from mladversarialobjectdetection_amd import detector as D
    bb, sc = D.filter_by_thresh([(0, 0, 1, 1), (1, 1, 2, 2), (2, 2, 3, 3)], [0.7, 0.5, 0.49], 0.5)
    assert bb == [(0, 0, 1, 1), (1, 1, 2, 2)] and sc == [0.7, 0.5]  # keeps >=
    with pytest.raises(ValueError, match="unsupported params key"):
        D.Detector(params={"num_classes": 3})
    with pytest.raises(ValueError, match="square"):
        D.Detector(params={"image_size": (480, 640)})
