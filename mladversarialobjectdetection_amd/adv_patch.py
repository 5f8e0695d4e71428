"""Inference-time patch compositor — mirror of the reference's adv_patch.py.

Reference: `AdversarialPatch` (adv_patch.py:16-201) pastes a printed, brightness-matched, resized and
noised copy of the adversarial patch onto every person box of an image with numpy + OpenCV on the
CPU (the demos call `add_adv_to_img(frame, boxes)`, demo.py:116, 177).  Here the same class drives
one HIP call, `phx_adv_patch` (csrc/kernels_advpatch.hip), over a whole batch of uint8 images on the
device (`phx_adv_patch_dev` when the boxes are device tensors, e.g. Detector.infer_device's: no
host round trip); the arithmetic follows OpenCV's own fixed-point / float32 steps and numpy's float64 ones
(restated in oracle/adv_patch.py, the tests' checker).  No CPU fallback: the library must be present.

Random draws: the reference's random patch (np.random.rand, :31) and the per-pixel noise
(np.random.uniform, :147) are Philox draws keyed by the context seed here, so a run is reproducible
and independent of the batch split.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

PATCH_SIZE = 640


def _stream():
    return torch.cuda.current_stream().cuda_stream


class AdversarialPatch:
    """adv_patch.AdversarialPatch: same constructor arguments (scale, h, w, patch_file) and the
    methods a caller uses — print_patch, add_adv_to_img — plus add_adv_to_images for a device batch.
    `seed` keys the random patch (when patch_file is None) and the noise; `ctx` lets several objects
    share one library context."""

    def __init__(self, *, scale, h=PATCH_SIZE, w=PATCH_SIZE, patch_file=None, seed=0, ctx=None, device="cuda"):
        if patch_file is not None:
            from PIL import Image
            self._patch_img = np.asarray(Image.open(patch_file).convert("RGB"))
        else:
            rng = np.random.default_rng(seed)
            self._patch_img = (rng.random((h, w, 3)) * 255).astype("uint8")
        if self._patch_img.shape[0] != self._patch_img.shape[1]:
            raise ValueError("AdversarialPatch: the patch must be square (the attacker writes 640x640)")
        self.scale = float(scale)
        self.seed = seed  # keys the noise (the context's seed when ctx is given)
        self.output_size = int(h), int(w)
        self.mean_rgb, self.stddev_rgb = 127.0, 128.0
        self.device = torch.device(device)
        self._ctx = ctx or _lib.Context("efficientdet-d0", 0, 1, seed=seed)
        self._patch_dev = torch.as_tensor(np.ascontiguousarray(self._patch_img), device=self.device)
        self._calls = 0

    def print_patch(self):
        """The printed patch (adv_patch.py:40-58; the library applies it to the stored patch)."""
        p = self._patch_img.astype(np.int64)
        return ((p + 127) >> 1).astype(np.uint8)

    def add_adv_to_images(self, images: torch.Tensor, bboxes, step=None, global_image_offset=0, *, count=None,
                          rounds=None):
        """add_adv_to_img for a batch: images [B,H,W,3] uint8 on the device (a patched copy is returned),
        bboxes[b] = the person boxes (ymin, xmin, ymax, xmax) of image b, taken as float32 (the
        detector's output dtype; _create's arithmetic then follows numpy's promotion of float32).

        Device boxes: bboxes a float32 device tensor [B,max_boxes,4] with count [B] int32 on the device
        (Detector.infer_device's pboxes / pcount) goes through phx_adv_patch_dev and returns
        (images, status): status [B] int32 on the device holds the _lib.AP_* bits of what was not pasted
        (what the host-list path raises for).  rounds = the paste rounds to issue; None reads
        count.max() back (the call's one host round trip)."""
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("add_adv_to_images: expected [B,H,W,3] uint8")
        B, H, W, _ = images.shape
        if torch.is_tensor(bboxes):
            if count is None or not torch.is_tensor(count):
                raise ValueError("add_adv_to_images: device boxes need a device count tensor")
            if bboxes.dtype != torch.float32 or bboxes.dim() != 3 or bboxes.shape[0] != B or bboxes.shape[2] != 4:
                raise ValueError("add_adv_to_images: device boxes must be float32 [B,max_boxes,4]")
            if count.dtype != torch.int32 or tuple(count.shape) != (B,):
                raise ValueError("add_adv_to_images: device count must be int32 [B]")
            if bboxes.device != images.device or count.device != images.device:
                raise ValueError("add_adv_to_images: images, boxes and count must share a device")
            bboxes, count = bboxes.contiguous(), count.contiguous()
            if rounds is None:
                rounds = min(max(int(count.max().item()), 0), int(bboxes.shape[1]))
            out = images.contiguous().clone()
            status = torch.empty(B, dtype=torch.int32, device=images.device)
            if step is None:
                step = self._calls
            self._calls += 1
            oh, ow = self.output_size
            self._ctx.call("phx_adv_patch_dev", out.data_ptr(), B, H, W, bboxes.data_ptr(), count.data_ptr(),
                           int(bboxes.shape[1]), int(rounds), self._patch_dev.data_ptr(), int(self._patch_dev.shape[0]),
                           self.scale, oh, ow, int(step), int(global_image_offset), status.data_ptr(), _stream())
            return out, status
        if count is not None or rounds is not None:
            raise ValueError("add_adv_to_images: count / rounds go with device boxes")
        if len(bboxes) != B:
            raise ValueError("add_adv_to_images: one box list per image")
        out = images.contiguous().clone()
        counts = np.asarray([len(bb) for bb in bboxes], dtype=np.int32)
        maxb = max(1, int(counts.max()) if B else 1)
        boxes = np.zeros((B, maxb, 4), dtype=np.float32)
        for b, bb in enumerate(bboxes):
            if len(bb):
                boxes[b, :len(bb)] = np.asarray(bb, dtype=np.float32).reshape(-1, 4)
        if step is None:
            step = self._calls
        self._calls += 1
        oh, ow = self.output_size
        self._ctx.call("phx_adv_patch", out.data_ptr(), B, H, W, boxes.ctypes.data, counts.ctypes.data, maxb,
                       self._patch_dev.data_ptr(), int(self._patch_dev.shape[0]), self.scale, oh, ow, int(step),
                       int(global_image_offset), _stream())
        return out

    def add_adv_to_img(self, img: np.ndarray, bboxes, step=None):
        """adv_patch.py:189-201: the patched copy of one HxWx3 uint8 image (host in, host out)."""
        t = torch.as_tensor(np.ascontiguousarray(img), device=self.device)[None]
        return self.add_adv_to_images(t, [list(bboxes)], step=step)[0].cpu().numpy()
