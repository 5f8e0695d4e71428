"""Frame recovery restated for the tests (a helper, not a test): RecoveryDemo.serve (demo_v2.py:151-169)
and run's uint8 cast (:134) in fp64 arithmetic on the fp32 constants and fp32 interpolation weights,
built from serve_oracle.preprocess64, oracle.defender.UNet(training=False) and
oracle.data.cv2_resize_linear.  cv2 and TensorFlow are not importable here: their arithmetic is the
restatement of oracle/data.py and oracle/eot.py [recall].
"""
import numpy as np
import torch

import serve_oracle as so
from oracle import data as OD
from oracle import defender as DF

f32 = np.float32
EPS = 8 * 2.0 ** -24 * 256  # one rounding per product and sum of the two passes and the denormalise, at <= 256


def side(h, w, S):
    """d = int(fp32(S) * image_scale_to_original): cv2.resize's destination side (demo_v2.py:163-165)."""
    return int(f32(f32(S) * so.scale_to_original(h, w, S)))


def dims(h, w, S):
    """(h', w') of the recovered frame: the d x d resize cropped to [:h, :w].  Raises where the
    reference's resizes do (an empty size)."""
    if h < 1 or w < 1:
        raise ValueError("empty frame")
    sh, sw, _ = so.dims(h, w, S)
    d = side(h, w, S)
    if sh < 1 or sw < 1 or d < 1:
        raise ValueError("empty resize")
    return min(h, d), min(w, d)


def epilogue(canvas, updates, h, w, S, mean, std):
    """Steps 2-5 over a canvas x and updates = 2 * PatchNeutralizer(x), both [S,S,3]:
    clip(updates + x, -1, 1) * stddev_rgb + mean_rgb, cv2.resize to (d, d), crop -> float64 [h',w',3]."""
    y = np.clip(np.asarray(updates, np.float64) + np.asarray(canvas, np.float64), -1.0, 1.0)
    y = y * np.asarray(std, f32).astype(np.float64) + np.asarray(mean, f32).astype(np.float64)
    d = side(h, w, S)
    oh, ow = dims(h, w, S)
    return OD.cv2_resize_linear(y, d, d)[:oh, :ow]


def to_uint8(img):
    """np.clip(., 0, 255).astype('uint8') (demo_v2.py:134): the cast truncates."""
    return np.clip(img, 0.0, 255.0).astype(np.uint8)


def near_integer(img, eps=EPS):
    """Pixels whose uint8 value a rounding of size eps can change: within eps of one of the cast's
    thresholds 1..255 (below 1 - eps and above 255 + eps the clip decides)."""
    v = np.asarray(img, np.float64)
    return (np.abs(v - np.rint(v)) <= eps) & (v >= 1.0 - eps) & (v <= 255.0 + eps)


def unet64(params, moving, canvases, dtype=torch.float64):
    """2 * PatchNeutralizer(x, training=False) in `dtype` for canvases [B,S,S,3]: params the flat
    variables, moving the oracle's {BN name: (mean, variance)}."""
    layout, _ = DF.unet_layout()
    net = DF.UNet(DF.unpack(np.asarray(params), layout), moving, dtype=dtype, training=False)
    with torch.no_grad():
        out = net(torch.as_tensor(np.asarray(canvases), dtype=dtype))
    return 2.0 * out.numpy().astype(np.float64)


def serve64(frame, S, mean, std, params, moving):
    """The whole chain for one uint8 frame -> (float64 image [h',w',3], canvas, updates)."""
    h, w, _ = frame.shape
    x = so.preprocess64(frame, S, mean, std)
    u = unet64(params, moving, x[None])[0]
    return epilogue(x, u, h, w, S, mean, std), x, u
