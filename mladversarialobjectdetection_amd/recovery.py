"""Frame recovery with the trained defender U-Net — mirror of the reference's RecoveryDemo
(demo_v2.py:99-169, demo.py:167-219) over libphx, without the cv2 drawing, text overlay and video I/O.

  Recovery.serve    RecoveryDemo.serve (demo_v2.py:151-169): attacked uint8 frames -> the recovered
                    float images at frame size
  Recovery.recover  the same followed by run's np.clip(., 0, 255).astype('uint8') (:134), left on the
                    device as detector.PackedFrames, so Detector.infer_batch / ServeDriver.serve take
                    it without a host round trip
  Recovery.run      RecoveryDemo.run (:124-149): paste the patch, recover, detect, compare scores

Everything runs in libphx.so (phx_adv_patch, phx_def_recover, phx_serve) on the current PyTorch-ROCm
stream; there is no CPU fallback.  A recovered frame can be one row or column smaller than its input:
the reference resizes to d = int(fp32(image_size) * image_scale_to_original), a truncating fp32
product that is sometimes one less than the frame's longer side (include/phx.h).
"""
from __future__ import annotations

import numpy as np
import torch

from .defender import PatchAttackDefender
from .detector import Detector, PackedFrames, filter_by_thresh

SCORE_THRESH = .55  # demo_v2.py:28


def unpack_frames(p: PackedFrames, data: torch.Tensor = None):
    """The frames of a PackedFrames as a list of host [h,w,3] arrays (`data`: another packed tensor
    with the same element offsets, e.g. the float images)."""
    flat = (p.src if data is None else data).cpu().numpy()
    return [flat[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(p.offsets.tolist(), p.dims.tolist())]


class Recovery:
    """RecoveryDemo: `weights` is anything PatchAttackDefender(initial_weights=...) accepts (an
    antipatch.h5, a save_weights directory, an .npz, a flat array; None = freshly initialised),
    `patch` an adv_patch.AdversarialPatch, `detector` the Detector whose victim context the U-Net is
    built on (at its image size, for batches up to its max_batch)."""

    def __init__(self, weights, patch, detector: Detector, *, min_score_thresh=SCORE_THRESH,
                 atk_detection_thresh=10., seed=0):
        self.patch_obj = patch
        self.dct_obj = detector
        self.config = detector.driver.model.config
        self.min_score_thresh = min_score_thresh
        self.atk_detection_thresh = atk_detection_thresh
        self.defender = PatchAttackDefender(detector.driver.model, initial_weights=weights, seed=seed)

    def recover(self, frames) -> PackedFrames:
        """Attacked uint8 frames -> the recovered uint8 frames, packed on the device."""
        return self.defender.recover(frames)[0]

    def serve(self, frames):
        """RecoveryDemo.serve for every frame: a list of float32 [h', w', 3] arrays."""
        packed, floats = self.defender.recover(frames, uint8=True, float32=True)
        return unpack_frames(packed, floats)

    def run(self, frame, bb, sc, osc):
        """RecoveryDemo.run (demo_v2.py:124-149) without the drawing: frame with person boxes bb, sc /
        osc the best person score (percent) after / before the attack.  -> (recovered frame uint8, its
        person boxes, its best person score in percent, attack_detected)."""
        mal_frame = self.patch_obj.add_adv_to_img(np.asarray(frame), bb)
        packed = self.recover([mal_frame])
        recovered = unpack_frames(packed)[0]
        bb_after, sc_after = self.dct_obj.infer_batch(packed)[0]
        bb_after, sc_after = filter_by_thresh(bb_after, sc_after, self.min_score_thresh)
        sc_after = max(sc_after) * 100. if len(sc_after) else 0.
        thresh = int(self.min_score_thresh * 100.)
        attack_detected = bool(osc > thresh and sc_after - sc > self.atk_detection_thresh)
        return recovered, bb_after, sc_after, attack_detected
