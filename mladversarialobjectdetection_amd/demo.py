"""The demos' loop on the device — mirror of the reference's demo.py (:29-219 the three demo classes,
:276-378 main's loop; demo_v2.py:192- is the same loop with less bookkeeping).

The reference takes a learned patch and a trained defender and runs a clip four ways — clean,
adversarial patch, random patch as the baseline, recovery — and overlays the best person score of each
run, their running means, the attack success rate and the attack detection rate.  Here:

  Demo / AttackDemo / RecoveryDemo   the reference's bookkeeping only: measure_mean_score (demo.py:51-59),
                                     calc_asr (:98-105, the queue rule of :123-125), calc_adr (:159-165,
                                     the queue rule of :187-190)
  ClipEvaluator                      main's loop (:336-342) over a whole clip in batches of the
                                     detector's max_batch, without a host round trip per frame:
                                     phx_serve + phx_persons (Detector.infer_device), phx_adv_patch_dev
                                     (AdversarialPatch.add_adv_to_images with device boxes),
                                     phx_def_recover (Recovery.recover); the scores are read back once,
                                     at the end of the clip, and fed to the three classes in frame order;
                                     run_stream takes the raw frames of a streaming.Stream, resized on
                                     the device as the demos' Stream does (demo.py:284, demo_v2.py:202)

Arithmetic of the bookkeeping: a frame's score is its best person score as float32 times float32(100)
(the reference's np.float32 * 100. under NumPy's scalar promotion), the threshold is
int(min_score_thresh * 100.), rates and means go through Python's round (half to even).  One deliberate
deviation: the running mean is taken in float64 over the float32 scores (the reference's np.mean runs in
float32 until the first frame without a person appends a Python 0., and in float64 from then on).

calc_asr / calc_adr on an empty queue (no frame with a clean detection above the threshold yet) return
None; the reference divides by zero there and only ever calls them after an append, as ClipEvaluator does.

Out of scope: cv2 drawing and text, make_graph, the 2x2 mosaic, video decode, the webcam and the
VideoWriter (streaming's resize is streaming.py's Stream), demo_v2's flash colour.  There is no CPU fallback: the library must be present.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .detector import PackedFrames

SCORE_THRESH = .55  # demo.py:26


class Demo:
    """demo.Demo's bookkeeping: the scores seen so far and their running mean."""

    def __init__(self, name, *, min_score_thresh=SCORE_THRESH):
        self.name = name
        self._sc_arr = []
        self.min_score_thresh = min_score_thresh

    @property
    def thresh(self):
        return int(self.min_score_thresh * 100.)

    def measure_mean_score(self, sc):
        """demo.py:51-59: sc = the person scores of one frame (any sequence; empty = no person) ->
        the rounded mean over all frames so far of the per-frame maximum, in percent."""
        max_sc = np.float32(max(sc)) if len(sc) else np.float32(0.)
        self._sc_arr.append(max_sc)
        return round(np.mean(np.asarray(self._sc_arr, np.float64)) * 100.)

    def run(self, sc):
        """Demo.run without the inference and the drawing (demo.py:72-81): sc as measure_mean_score ->
        (mean score so far, this frame's best score in percent as float32)."""
        mean_sc = self.measure_mean_score(sc)
        return mean_sc, (np.float32(max(sc)) * np.float32(100.) if len(sc) else np.float32(0.))


class AttackDemo(Demo):
    """demo.AttackDemo's bookkeeping: the attacked scores of the frames whose clean score exceeded the
    threshold, and the share of them below it."""

    def __init__(self, name, *, min_score_thresh=SCORE_THRESH):
        super().__init__(name, min_score_thresh=min_score_thresh)
        self._atk_queue = []

    def calc_asr(self):
        """demo.py:98-105 (None while the queue is empty)."""
        if not self._atk_queue:
            return None
        thresh = self.thresh
        success = len([x for x in self._atk_queue if x < thresh])
        return round(success / len(self._atk_queue) * 100.)

    def run(self, sc, osc):
        """AttackDemo.run after the paste (demo.py:119-134): sc = the attacked frame's person scores,
        osc = the clean frame's score in percent -> (mean score, attacked score in percent, counted,
        attack_success); attack_success is False for a frame that is not counted."""
        mean_sc, sc = super().run(sc)
        thresh = self.thresh
        counted = bool(sc > -1. and osc > thresh)
        if counted:
            self._atk_queue.append(sc)
        return mean_sc, sc, counted, bool(counted and sc < thresh)


class RecoveryDemo(Demo):
    """demo.RecoveryDemo's bookkeeping: the score recovered by the defender on the frames whose clean
    score exceeded the threshold, and the share of them above atk_detection_thresh.  (The U-Net itself
    is recovery.Recovery.)"""

    def __init__(self, name, *, min_score_thresh=SCORE_THRESH, atk_detection_thresh=10.):
        super().__init__(name, min_score_thresh=min_score_thresh)
        self._diff_queue = []
        self.atk_detection_thresh = atk_detection_thresh

    def calc_adr(self):
        """demo.py:159-165 (None while the queue is empty)."""
        if not self._diff_queue:
            return None
        success = len([x for x in self._diff_queue if x > self.atk_detection_thresh])
        return round(success / len(self._diff_queue) * 100.)

    def run(self, sc_after, sc, osc):
        """RecoveryDemo.run after the recovery (demo.py:183-199): sc_after = the recovered frame's person
        scores, sc / osc = the score after / before the attack in percent -> (mean score, recovered
        score in percent, counted, attack_detected); an attack counts as detected when the recovered
        score exceeds the attacked one by more than atk_detection_thresh (calc_adr's rule)."""
        mean_sc, sc_after = super().run(sc_after)
        counted = bool(osc > self.thresh)
        detected = False
        if counted:
            score_recovery = sc_after - np.float32(sc)
            self._diff_queue.append(score_recovery)
            detected = bool(score_recovery > self.atk_detection_thresh)
        return mean_sc, sc_after, counted, detected


@dataclass
class ClipResult:
    """What demo.py overlays, per frame of the clip (lists of length N) and at its end."""
    sc_clean: np.ndarray            # float32 [N] best person score in percent, clean frames
    sc_random: np.ndarray           # ... with the random patch
    sc_before: np.ndarray           # ... with the adversarial patch (before the recovery)
    sc_after: np.ndarray            # ... after the recovery
    counted: np.ndarray             # bool [N]: the clean score exceeded the threshold (the frame is in the queues)
    attack_success: np.ndarray      # bool [N]: counted and sc_before below the threshold
    attack_success_random: np.ndarray
    attack_detected: np.ndarray     # bool [N]: counted and sc_after - sc_before above atk_detection_thresh
    mean_score: dict = field(default_factory=dict)  # {"clean" | "random" | "attack" | "recovery": [N] ints}
    asr: list = field(default_factory=list)         # after each frame (None until a frame is counted)
    asr_random: list = field(default_factory=list)
    adr: list = field(default_factory=list)
    status: np.ndarray = None       # int32 [3,N]: phx_adv_patch_dev's status of the three composites (all zero)
    attacked: torch.Tensor = None   # uint8 [N,h,w,3] on the device (keep_frames=True)
    attacked_random: torch.Tensor = None
    recovered: list = None          # per batch: detector.PackedFrames on the device (keep_frames=True)

    @property
    def final(self):
        last = lambda a: a[-1] if len(a) else None
        return {"asr": last(self.asr), "asr_random": last(self.asr_random), "adr": last(self.adr),
                "mean_score": {k: last(v) for k, v in self.mean_score.items()}}


_BITS = ((_lib.AP_REFUSED, "a person box gives a patch below one pixel or larger than the frame"),
         (_lib.AP_OVERFLOW, "more person boxes than paste rounds"),
         (_lib.AP_BADCOUNT, "box count out of range"))


class ClipEvaluator:
    """main's loop (demo.py:276-378) for a clip: `detector` a detector.Detector, `patch` / `rand_patch`
    adv_patch.AdversarialPatch objects (the learned patch, the random baseline), `recovery` a
    recovery.Recovery.  The three bookkeeping objects live as long as the evaluator, so the rates and
    means run on over several clips, as the reference's do over its stream.

    Noise keys: the composites of the evaluator's c-th clip use step 3c (adversarial), 3c + 1 (random)
    and 3c + 2 (the recovery's fresh paste, demo.py:177) with global_image_offset = the frame's index in
    the clip, so the result does not depend on max_batch."""

    def __init__(self, detector, patch, rand_patch, recovery, *, min_score_thresh=SCORE_THRESH,
                 atk_detection_thresh=10., max_batch=None):
        """max_batch: frames per batch, at most (and by default) the detector's max_batch."""
        self.dct_obj = detector
        cap = detector.driver.model.max_batch
        self.max_batch = cap if max_batch is None else int(max_batch)
        if not 1 <= self.max_batch <= cap:
            raise ValueError(f"ClipEvaluator: max_batch {max_batch} outside [1, the detector's {cap}]")
        self.patch_obj, self.rand_patch_obj, self.recovery = patch, rand_patch, recovery
        self.min_score_thresh = min_score_thresh
        self.demo_clean = Demo("clean", min_score_thresh=min_score_thresh)
        self.demo_patch = AttackDemo("adv. patch", min_score_thresh=min_score_thresh)
        self.demo_rnd_patch = AttackDemo("random patch (as baseline)", min_score_thresh=min_score_thresh)
        self.demo_recovery = RecoveryDemo("recovery", min_score_thresh=min_score_thresh,
                                          atk_detection_thresh=atk_detection_thresh)
        self.clips = 0

    def _packed(self, batch):
        n, h, w, _ = batch.shape
        return PackedFrames(batch.reshape(-1), np.arange(n, dtype=np.int64) * (h * w * 3),
                            np.tile(np.asarray([[h, w]], np.int32), (n, 1)))

    def run_stream(self, stream, *, rounds=None, keep_frames=False) -> ClipResult:
        """`run` on the frames of a streaming.Stream: raw frames of any size, resized on the device to the
        stream's set_width in batches of max_batch (one upload and one phx_ingest each; a stream without a
        ctx uses the detector's) and gathered into one device [N,dh,dw,3] tensor — 3 * dh * dw bytes of
        device memory per frame of the clip, held until `run` returns.  The demos assume one frame size
        (np.concatenate, a VideoWriter sized from the first frame): a frame whose ingested size differs
        from the first's raises ValueError naming its index, before any bookkeeping object is touched."""
        from .streaming import unpack_device
        ctx = stream.ctx or self.dct_obj.driver.model.ctx
        clip, first, i = [], None, 0
        for p in stream.batches(self.max_batch, ctx=ctx):
            for (dh, dw), fr in zip(p.dims, unpack_device(p)):
                first = first or (int(dh), int(dw))
                if (int(dh), int(dw)) != first:
                    raise ValueError(f"ClipEvaluator.run_stream: frame {i} is {int(dh)}x{int(dw)} after the ingest, "
                                     f"the clip's first frame {first[0]}x{first[1]}")
                clip.append(fr)
                i += 1
        if not clip:
            raise ValueError("ClipEvaluator.run_stream: the stream has no frames")
        return self.run(torch.stack(clip), rounds=rounds, keep_frames=keep_frames)

    def run(self, frames, *, rounds=None, keep_frames=False) -> ClipResult:
        """frames [N,h,w,3] uint8 (numpy or a device tensor).  rounds: the paste rounds per batch (an
        upper bound of the thresholded persons per frame); None reads each batch's largest count back.
        A box that could not be pasted (phx_adv_patch_dev's status) raises PhxError after the clip."""
        victim = self.dct_obj.driver.model
        dev = torch.device("cuda", victim.device)
        frames = torch.as_tensor(frames).to(dev)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.shape[0]:
            raise ValueError("ClipEvaluator.run: expected [N,h,w,3] uint8 frames")
        frames = frames.contiguous()
        N, mb, c = frames.shape[0], self.max_batch, self.clips
        self.clips += 1
        thr = self.min_score_thresh
        best = torch.zeros(4, N, device=dev)
        status = torch.zeros(3, N, dtype=torch.int32, device=dev)
        kept = ([], [], [])
        for i0 in range(0, N, mb):
            sl = slice(i0, min(i0 + mb, N))
            batch = frames[sl]
            pboxes, pcount, best[0, sl] = self.dct_obj.infer_device(self._packed(batch), thr)
            r = int(rounds) if rounds is not None else min(max(int(pcount.max().item()), 0), _lib.MAX_OUT)
            paste = dict(count=pcount, rounds=r, global_image_offset=i0)
            mal, status[0, sl] = self.patch_obj.add_adv_to_images(batch, pboxes, step=3 * c, **paste)
            ctrl, status[1, sl] = self.rand_patch_obj.add_adv_to_images(batch, pboxes, step=3 * c + 1, **paste)
            mal2, status[2, sl] = self.patch_obj.add_adv_to_images(batch, pboxes, step=3 * c + 2, **paste)
            best[2, sl] = self.dct_obj.infer_device(self._packed(mal), thr)[2]
            best[1, sl] = self.dct_obj.infer_device(self._packed(ctrl), thr)[2]
            rec = self.recovery.recover(self._packed(mal2))
            best[3, sl] = self.dct_obj.infer_device(rec, thr)[2]
            if keep_frames:
                for lst, x in zip(kept, (mal, ctrl, rec)):
                    lst.append(x)
        best, status = best.cpu().numpy(), status.cpu().numpy()  # the clip's one readback
        bad = np.argwhere(status != 0)
        if len(bad):
            k, i = (int(v) for v in bad[0])
            why = "; ".join(msg for bit, msg in _BITS if status[k, i] & bit)
            raise _lib.PhxError(f"ClipEvaluator.run: frame {i}, composite {('adversarial', 'random', 'recovery')[k]}: "
                                f"{why} (status {int(status[k, i])})")
        res = ClipResult(*(np.zeros(N, np.float32) for _ in range(4)), *(np.zeros(N, bool) for _ in range(4)),
                         mean_score={k: [] for k in ("clean", "random", "attack", "recovery")}, status=status)
        for i in range(N):
            # demo.py:337-342; a frame without a person has best = 0, the reference's empty score list
            sc = [[best[k, i]] if best[k, i] > 0 else [] for k in range(4)]
            m_clean, res.sc_clean[i] = self.demo_clean.run(sc[0])
            m_atk, res.sc_before[i], res.counted[i], res.attack_success[i] = self.demo_patch.run(sc[2], res.sc_clean[i])
            m_rnd, res.sc_random[i], _, res.attack_success_random[i] = self.demo_rnd_patch.run(sc[1], res.sc_clean[i])
            m_rec, res.sc_after[i], _, res.attack_detected[i] = self.demo_recovery.run(sc[3], res.sc_before[i],
                                                                                      res.sc_clean[i])
            for k, m in zip(("clean", "random", "attack", "recovery"), (m_clean, m_rnd, m_atk, m_rec)):
                res.mean_score[k].append(m)
            res.asr.append(self.demo_patch.calc_asr())
            res.asr_random.append(self.demo_rnd_patch.calc_asr())
            res.adr.append(self.demo_recovery.calc_adr())
        if keep_frames:
            res.attacked, res.attacked_random = torch.cat(kept[0]), torch.cat(kept[1])
            res.recovered = kept[2]
        return res
