"""The serving path's pre- and post-processing restated for the tests (a helper, not a test):
EfficientDetModel.call(raw_frames, training=False, pre_mode='infer', post_mode='global')
(automl/efficientdet/tf2/efficientdet_keras.py:912-994) around the detector forward.  Built from the
oracle's pieces: oracle.eot.resize_matrix (tf.image.resize(antialias=True) per axis),
oracle.detector.pre_nms and oracle.postprocess.soft_nms (NonMaxSuppressionV5).
"""
import numpy as np

from oracle import eot
from oracle import postprocess as pp

f32 = np.float32
CLASS_OFFSET = 1  # postprocess.py:30
MAX_OUT = 100     # nms_configs.max_output_size, hparams_config.py:264


def dims(h, w, S):
    """InputProcessor.set_scale_factors_to_output_size (dataloader.py:115-127) in fp32:
    -> (scaled_h, scaled_w, image_scale); the scaled sides are truncating fp32 products."""
    sy = f32(f32(S) / f32(h))
    sx = f32(f32(S) / f32(w))
    s = min(sx, sy)
    return int(f32(f32(h) * s)), int(f32(f32(w) * s)), s


def scale_to_original(h, w, S):
    """DetectionInputProcessor.image_scale_to_original (dataloader.py:199-201): 1 / image_scale, fp32."""
    return f32(f32(1.0) / dims(h, w, S)[2])


def preprocess64(frame, S, mean, std):
    """_preprocessing(mode='infer') of one uint8 frame [h,w,3] (efficientdet_keras.py:925-936 ->
    dataloader.py:59-65 normalize_image, :129-142 resize_and_crop_image + pad_to_bounding_box) in
    fp64 arithmetic on the fp32 constants and fp32 weight matrices: -> [S,S,3] float64."""
    h, w, _ = frame.shape
    sh, sw, _ = dims(h, w, S)
    x = (frame.astype(np.float64) - np.asarray(mean, f32).astype(np.float64)) / np.asarray(std, f32).astype(np.float64)
    Wy = eot.resize_matrix(sh, h).astype(np.float64)
    Wx = eot.resize_matrix(sw, w).astype(np.float64)
    y = np.einsum("ih,hwc->iwc", Wy, x)
    y = np.einsum("jw,iwc->ijc", Wx, y)
    out = np.zeros((S, S, 3))
    out[:sh, :sw] = y
    return out


def taps(h, w, S):
    """(T_y, T_x): the largest number of non-zero weights in a row of each axis' resize matrix."""
    sh, sw, _ = dims(h, w, S)
    return (int((eot.resize_matrix(sh, h) != 0).sum(1).max()), int((eot.resize_matrix(sw, w) != 0).sum(1).max()))


def postprocess_global(boxes, scores, classes, S, nms_thresh, scale=None):
    """postprocess_global (postprocess.py:375-406) for one image after pre_nms: nms(padded=True)
    (:159-205, gaussian, sigma 0.5 -> NonMaxSuppressionV5 with soft_nms_sigma 0.25, score threshold
    `score_thresh or 0.001`) on every candidate, clip_boxes to [0, S] (:61-64), then x
    image_scale_to_original in fp32 (:398-400), classes + CLASS_OFFSET as float32 (:203, :30).
    -> (boxes [100,4], scores [100], classes [100], n) float32; rows >= n are zero (the library's
    deliberate departure from TF's padded output, which repeats candidate 0 there)."""
    boxes = np.asarray(boxes, f32)
    scores = np.asarray(scores, f32)
    idx, sc = pp.soft_nms(boxes, scores, MAX_OUT, nms_thresh, 0.5 / 2)
    n = len(idx)
    ob = np.zeros((MAX_OUT, 4), f32)
    os_ = np.zeros(MAX_OUT, f32)
    oc = np.zeros(MAX_OUT, f32)
    if n:
        b = np.clip(boxes[idx], f32(0), f32(S)).astype(f32)
        if scale is not None:
            b = (b * f32(scale)).astype(f32)
        ob[:n] = b
        os_[:n] = sc
        oc[:n] = (np.asarray(classes)[idx] + CLASS_OFFSET).astype(f32)
    return ob, os_, oc, n
