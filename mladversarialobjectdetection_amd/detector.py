"""Serving raw frames — mirror of the reference's detector.Detector (detector.py:19-60) over libphx.

  Detector.infer           detector.py:35-60: one raw uint8 frame of any size -> person boxes in
                           frame pixels and their scores, in NMS order
  Detector.infer_device    the same followed by util.filter_by_thresh and the demos' max(sc)
                           (demo.py:72-81), left on the device (phx_serve + phx_persons)
  ServeDriver.serve        infer_lib.KerasDriver.serve (infer_lib.py:408-421) ->
                           EfficientDetModel.call(raw_frames, training=False, pre_mode='infer',
                           post_mode='global') (efficientdet_keras.py:912-994)
  ServeDriver._preprocess  EfficientDetModel._preprocessing(mode='infer') (dataloader.py:59-201)
  filter_by_thresh         util.py:163-174

Everything runs in libphx.so (phx_serve / phx_serve_preprocess / phx_nms_global / phx_persons) on the current
PyTorch-ROCm stream; there is no CPU fallback.  One deliberate difference: rows at and beyond
valid_len are zero in every output (TF's padded NonMaxSuppressionV5 repeats candidate 0 there and
detector.py:51-57 loops over all 100 rows); `infer` reads the first valid_len rows only.
Not mirrored: __call__ (cv2 drawing).  The demos' loop is demo.py's ClipEvaluator, their stream's resize
streaming.py's Stream.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .attacker import EfficientDetVictim, _stream

MODEL = "efficientdet-lite4"  # detector.py:15


class PackedFrames(NamedTuple):
    """A batch of HWC uint8 frames in one device buffer; offsets / dims stay on the host (the
    library validates them before it launches anything)."""
    src: torch.Tensor      # uint8 [sum h*w*3], device
    offsets: np.ndarray    # int64 [B] byte offsets into src
    dims: np.ndarray       # int32 [B,2] (h, w)


def pack_frames(frames, device) -> PackedFrames:
    """numpy uint8 [h,w,3] frames (one array, a [B,h,w,3] array or a list that may mix sizes) ->
    PackedFrames.  The tuple data.pack_images returns (device offsets / dims) is accepted too: its
    tables are copied back to the host."""
    if isinstance(frames, PackedFrames):
        return frames
    if isinstance(frames, tuple) and len(frames) == 3 and torch.is_tensor(frames[0]):
        src, off, dims = frames
        return PackedFrames(src.contiguous(), np.ascontiguousarray(torch.as_tensor(off).cpu().numpy(), np.int64),
                            np.ascontiguousarray(torch.as_tensor(dims).cpu().numpy(), np.int32).reshape(-1, 2))
    if isinstance(frames, np.ndarray):
        frames = [frames] if frames.ndim == 3 else list(frames)
    frames = list(frames)
    if not frames:
        raise ValueError("pack_frames: no frames")
    for fr in frames:
        if not isinstance(fr, np.ndarray) or fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError("pack_frames: expected HxWx3 uint8 frames")
    sizes = [int(fr.size) for fr in frames]
    offsets = np.zeros(len(frames), np.int64)
    offsets[1:] = np.cumsum(sizes)[:-1]
    flat = np.concatenate([np.ascontiguousarray(fr).reshape(-1) for fr in frames])
    dims = np.asarray([fr.shape[:2] for fr in frames], np.int32).reshape(-1, 2)
    return PackedFrames(torch.as_tensor(flat).to(device), offsets, dims)


class ServeDriver:
    """What Detector.driver exposes of infer_lib.KerasDriver: serve, the model and its config."""

    def __init__(self, model: EfficientDetVictim):
        self.model = model

    def _pack(self, frames) -> PackedFrames:
        p = pack_frames(frames, torch.device("cuda", self.model.device))
        if not p.src.is_cuda or p.src.dtype != torch.uint8:
            raise ValueError("frames must be packed into a uint8 device tensor")
        return p

    def _preprocess(self, frames):
        """-> (images [B,S,S,3] float32, image_scale_to_original [B]) on the device."""
        p = self._pack(frames)
        B, S = len(p.offsets), self.model.ctx.image_size
        images = torch.empty(B, S, S, 3, device=p.src.device)
        scales = torch.empty(B, device=p.src.device)
        self.model.ctx.call("phx_serve_preprocess", p.src.data_ptr(), p.offsets.ctypes.data, p.dims.ctypes.data, B,
                            images.data_ptr(), scales.data_ptr(), _stream())
        return images, scales

    def serve(self, frames, post_mode=None):
        """-> (boxes [B,100,4] frame pixels, scores [B,100], classes [B,100] float32 (1 = person),
        valid_len [B] int32) on the device; rows >= valid_len are zero.  post_mode 'global' or 'per_class'
        (EfficientDetModel.call's; boxes are not clipped under 'per_class'); None: the context's."""
        if post_mode is not None and post_mode != self.model.ctx.get_post_mode():
            self.model.ctx.set_post_mode(post_mode)
        p = self._pack(frames)
        B, dev = len(p.offsets), p.src.device
        boxes = torch.empty(B, _lib.MAX_OUT, 4, device=dev)
        scores = torch.empty(B, _lib.MAX_OUT, device=dev)
        classes = torch.empty(B, _lib.MAX_OUT, device=dev)
        valid = torch.empty(B, dtype=torch.int32, device=dev)
        self.model.ctx.call("phx_serve", p.src.data_ptr(), p.offsets.ctypes.data, p.dims.ctypes.data, B,
                            boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(), valid.data_ptr(), None,
                            _stream())
        return boxes, scores, classes, valid

    def postprocess_global(self, boxes, scores, classes, count=None, scales=None, entry="phx_nms_global"):
        """postprocess.postprocess_global (postprocess.py:375-406) over [B,N,4] / [B,N] / [B,N] int32
        candidates (count [B]: valid candidates per row); scales [B] or None (model pixels)."""
        boxes = boxes.contiguous().float()
        scores = scores.contiguous().float()
        classes = classes.to(torch.int32).contiguous()
        B, N = scores.shape
        dev = scores.device
        if count is not None:
            count = count.to(torch.int32).contiguous()
        if scales is not None:
            scales = scales.contiguous().float()
        ob = torch.empty(B, _lib.MAX_OUT, 4, device=dev)
        os_ = torch.empty(B, _lib.MAX_OUT, device=dev)
        ocl = torch.empty(B, _lib.MAX_OUT, device=dev)
        oc = torch.empty(B, dtype=torch.int32, device=dev)
        self.model.ctx.call(entry, boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(),
                            count.data_ptr() if count is not None else None, B, N,
                            scales.data_ptr() if scales is not None else None, ob.data_ptr(), os_.data_ptr(),
                            ocl.data_ptr(), oc.data_ptr(), _stream())
        return ob, os_, ocl, oc

    def postprocess_per_class(self, boxes, scores, classes, count=None, scales=None):
        """postprocess.per_class_nms (postprocess.py:409-467) over the same arguments: NMS per class under the
        context's nms_configs, the max_output_size best of all classes, boxes x scales and not clipped."""
        return self.postprocess_global(boxes, scores, classes, count, scales, entry="phx_nms_per_class")


def _persons(boxes, scores, classes, n, max_boxes):
    """detector.py:48-57 over the first n (valid) rows: class 1 only, NMS order, at most max_boxes."""
    bb, sc = [], []
    for i in range(int(n)):
        if len(bb) == max_boxes:
            break
        if classes[i] == 1:
            bb.append(tuple(boxes[i].tolist()))
            sc.append(scores[i])
    return bb, sc


class Detector:
    """detector.Detector: person detections of raw frames.

    params is the reference's model_params dict: image_size (square; taken at construction and
    checked against the model table by the library, whose error surfaces) and nms_configs (through
    VictimConfig.override); any other key raises, as override does."""

    def __init__(self, *, params=None, model=MODEL, weights="synthetic", max_batch=1, post_mode="global",
                 **victim_kwargs):
        params = dict(params or {})
        image_size = params.pop("image_size", victim_kwargs.pop("image_size", 0))
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise ValueError("Detector: square image_size only")
            image_size = image_size[0]
        nms = params.pop("nms_configs", None)
        if params:
            raise ValueError(f"Detector: unsupported params key {sorted(params)[0]!r} (only image_size, nms_configs)")
        # hparams_config.py:258-266: score_thresh defaults to 0; the forward is inference-mode whatever bn_mode
        victim_kwargs.setdefault("score_thresh", 0.0)
        victim_kwargs.setdefault("bn_mode", "frozen")
        victim = EfficientDetVictim(model, weights, image_size=int(image_size), max_batch=max_batch, **victim_kwargs)
        if nms is not None:
            victim.config.override({"nms_configs": dict(nms)})
        if post_mode not in _lib.POST_MODES:
            raise ValueError(f"Detector: post_mode {post_mode!r}: 'global' or 'per_class'")
        self.post_mode = post_mode
        self.driver = ServeDriver(victim)

    def infer(self, frame, max_boxes=200):
        """One raw frame -> (bb, sc): person boxes as (ymin, xmin, ymax, xmax) tuples in frame pixels
        and their scores, Python lists in NMS order."""
        return self.infer_batch([np.asarray(frame)], max_boxes)[0]

    def infer_batch(self, frames, max_boxes=200, post_mode=None):
        """`infer` for every frame of a batch (<= max_batch) through one phx_serve call; post_mode None: the
        detector's."""
        boxes, scores, classes, valid = (t.cpu().numpy()
                                         for t in self.driver.serve(frames, post_mode or self.post_mode))
        return [_persons(boxes[b], scores[b], classes[b], valid[b], max_boxes) for b in range(len(valid))]

    def infer_device(self, frames, min_score_thresh):
        """`infer_batch` + filter_by_thresh without leaving the device: -> (pboxes [B,100,4] the person
        boxes with score >= float32(min_score_thresh) in NMS order, zero beyond pcount [B] int32;
        best [B] float32 the best person score of each frame, thresholded or not, 0 without a person:
        demo.py:81's max(sc) before the * 100.)."""
        boxes, scores, classes, valid = self.driver.serve(frames, self.post_mode)
        B, dev = valid.shape[0], valid.device
        pboxes = torch.empty(B, _lib.MAX_OUT, 4, device=dev)
        pcount = torch.empty(B, dtype=torch.int32, device=dev)
        best = torch.empty(B, device=dev)
        self.driver.model.ctx.call("phx_persons", boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(),
                                   valid.data_ptr(), B, float(min_score_thresh), pboxes.data_ptr(),
                                   pcount.data_ptr(), best.data_ptr(), _stream())
        return pboxes, pcount, best


def filter_by_thresh(bb, sc, score_thresh):
    """util.filter_by_thresh (util.py:163-174): keeps scores >= score_thresh."""
    inds = [s >= score_thresh for s in sc]
    return [b for b, k in zip(bb, inds) if k], [s for s, k in zip(sc, inds) if k]
