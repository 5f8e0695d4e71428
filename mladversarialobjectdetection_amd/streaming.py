"""Stream ingest — mirror of the reference's streaming.Stream (streaming.py:21-103) with the resize on
the device.

The reference resizes every frame to a fixed width before anything else sees it
(change_frame_size, :53-62): scale = set_width / w in float64, dh = int(h * scale) — a truncated
float64 product, not h * set_width // w: a 77x77 frame becomes 639x640 — and
cv2.resize(frame, (set_width, dh)) with the default INTER_LINEAR.  Here that is one phx_ingest launch
per batch of raw frames of any sizes (csrc/kernels_ingest.hip: copy / 2x box / 11-bit fixed-point
bilinear, exact against oracle/adv_patch.py::resize_linear_u8); set_width=0 means no rescaling.

  Stream.frames             the raw host frames: a directory (os.listdir, filter_func, sort_func,
                            PIL .convert('RGB'), :44-51, :87-93, without the sleep(1/24)) or any
                            iterable of HWC uint8 frames, which stands in for the video decoder
  Stream.change_frame_size  :53-62 for one frame or a batch -> detector.PackedFrames on the device
  Stream.batches            up to n frames at a time: one upload (pack_frames), one phx_ingest
  Stream.play               :95-103: one device [dh,dw,3] uint8 tensor per frame

Out of scope: video decode and the webcam (cv2.VideoCapture is absent: a video file and path=None
raise NotImplementedError; a caller with a decoder of their own passes its frames, with bgr=True if they
are BGR, the swap of :75).  There is no CPU fallback: the device methods need the library and a GPU.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .attacker import _stream
from .detector import PackedFrames, pack_frames


def ingest_dims(set_width, dims) -> np.ndarray:
    """phx_ingest_dims: (h, w) rows [B,2] -> the ingest sizes [B,2] int32 (host arithmetic, no GPU)."""
    dims = np.ascontiguousarray(np.asarray(dims, np.int32).reshape(-1, 2))
    out = np.zeros_like(dims)
    lib = _lib.load()
    rc = lib.phx_ingest_dims(int(set_width), dims.ctypes.data, len(dims), out.ctypes.data)
    if rc != 0:
        msg = lib.phx_last_error(None)
        raise _lib.PhxError(f"phx_ingest_dims failed ({rc}): {msg.decode() if msg else ''}")
    return out


def unpack_device(p: PackedFrames) -> list:
    """The frames of a PackedFrames as device views [h,w,3] of its buffer."""
    return [p.src[int(o):int(o) + int(h) * int(w) * 3].view(int(h), int(w), 3) for o, (h, w) in zip(p.offsets, p.dims)]


def _check_frame(fr) -> np.ndarray:
    fr = np.asarray(fr)
    if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
        raise ValueError(f"Stream: expected HxWx3 uint8 frames, got {fr.dtype} {fr.shape}")
    return fr


class Stream:
    """streaming.Stream: `path` a directory of images, or the frames themselves ([N,h,w,3] uint8, a
    list, any iterable of HWC uint8 frames).  filter_func / sort_func act on the directory's file names
    as the reference's do.  bgr: the frames are BGR (a decoder's), read as RGB.  ctx: the _lib.Context
    whose frame tables and device the ingest uses (its max_batch bounds one launch); None builds a small
    one at the first device call."""

    def __init__(self, path, *, filter_func=None, sort_func=None, set_width=640, bgr=False, ctx=None):
        if int(set_width) < 0:
            raise ValueError(f"Stream: set_width {set_width} is negative")
        self.set_width = int(set_width)
        self.bgr = bool(bgr)
        self.ctx = ctx
        self.path = path
        self.files = None
        if path is None:
            raise NotImplementedError("Stream: path=None is the reference's webcam (cv2.VideoCapture(0)); capture "
                                      "is out of scope, pass the frames as an iterable")
        if isinstance(path, (str, os.PathLike)):
            if os.path.isdir(path):
                self.files = os.listdir(path)
                if filter_func:
                    self.files = list(filter(filter_func, self.files))
                if sort_func:
                    self.files.sort(key=sort_func)
            elif os.path.isfile(path):
                raise NotImplementedError(f"Stream: {os.fspath(path)!r} is a file: video decode (cv2.VideoCapture) is "
                                          "out of scope, decode it yourself and pass the frames (bgr=True for BGR)")
            else:
                raise FileNotFoundError(f"Stream: no directory {os.fspath(path)!r}")

    def frames(self):
        """The raw host frames, uint8 [h,w,3] each, in stream order (no GPU needed)."""
        if self.files is not None:
            from PIL import Image
            for name in self.files:
                yield np.asarray(Image.open(os.path.join(self.path, name)).convert("RGB"))
        else:
            for fr in self.path:
                yield _check_frame(fr)

    def _context(self, ctx=None):
        ctx = ctx or self.ctx
        if ctx is None:
            ctx = self.ctx = _lib.Context("efficientdet-d0", 0, 16)
        return ctx

    def change_frame_size(self, frames, *, ctx=None) -> PackedFrames:
        """streaming.py:53-62 on the device: one frame [h,w,3], a batch [B,h,w,3], a list of frames of
        any sizes or a PackedFrames -> the resized frames, packed (dims = phx_ingest_dims').  More than
        the context's max_batch frames go through several launches into the same buffer."""
        ctx = self._context(ctx)
        dev = torch.device("cuda", ctx.device)
        p = pack_frames(frames, dev)
        if not p.src.is_cuda or p.src.dtype != torch.uint8:
            raise ValueError("Stream.change_frame_size: frames must be packed into a uint8 device tensor")
        offsets = np.ascontiguousarray(p.offsets, np.int64)
        dims = np.ascontiguousarray(p.dims, np.int32).reshape(-1, 2)
        B = len(offsets)
        out_dims = ingest_dims(self.set_width, dims)
        sizes = out_dims[:, 0].astype(np.int64) * out_dims[:, 1] * 3
        out_off = np.zeros(B, np.int64)
        out_off[1:] = np.cumsum(sizes)[:-1]
        out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=p.src.device)
        flags = _lib.INGEST_BGR if self.bgr else 0
        for i0 in range(0, B, ctx.max_batch):
            n = min(ctx.max_batch, B - i0)
            o, d, oo = offsets[i0:i0 + n], dims[i0:i0 + n], out_off[i0:i0 + n]
            ctx.call("phx_ingest", p.src.data_ptr(), o.ctypes.data, d.ctypes.data, n, self.set_width, flags,
                     out.data_ptr(), oo.ctypes.data, _stream())
        return PackedFrames(out, out_off, out_dims)

    def batches(self, n, *, ctx=None):
        """PackedFrames of up to n ingested frames at a time, in stream order: one upload and one
        phx_ingest per batch (n <= the context's max_batch)."""
        n = int(n)
        if n < 1:
            raise ValueError(f"Stream.batches: n = {n} must be >= 1")
        ctx = self._context(ctx)
        pending = []
        for fr in self.frames():
            pending.append(fr)
            if len(pending) == n:
                yield self.change_frame_size(pending, ctx=ctx)
                pending = []
        if pending:
            yield self.change_frame_size(pending, ctx=ctx)

    def play(self, *, ctx=None):
        """streaming.py:95-103: one resized frame at a time, a device uint8 tensor [dh,dw,3] (a view of
        its batch's buffer; frames are ingested max_batch at a time)."""
        ctx = self._context(ctx)
        for p in self.batches(ctx.max_batch, ctx=ctx):
            yield from unpack_device(p)
