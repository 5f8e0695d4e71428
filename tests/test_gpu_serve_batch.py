"""GPU: an image's served result does not depend on the batch it was served in, end to end.

A frozen Detector with synthetic weights; mixed-size random frames preprocessed once; then phx_detect's dense
outputs (scores, classes and boxes over every anchor) and all four phx_serve outputs at score_thresh = 0.0 (100
rows per frame) are compared per image, bit for bit, between single-image calls and batches:

  D0 at 128^2   1, 4, 8, 16 frames per call and the 16 in a second order: se_plan(B, ...) moved at 8 and at 16
  D0 at 512^2   1, 4: the production size, whose levels plan the deep-K, A-resident and many-tile GEMM classes
                that 128^2 (few tiles everywhere) never does
  D4 at 256^2   1, 3, 4: a backbone whose SE slicing moved at B = 4 (tests/test_gpu_deep.py's context size)

tests/test_gpu_serve.py::test_infer_batch_equals_per_frame_infer keeps the person boxes above 0.5 at B = 4; this
module is the general claim of DESIGN.md section 15 ("Batch size").  On a mismatch the message names the first
differing op of the program, found through phx_debug_tap over the batch norms' names (each tap is a BN's input,
i.e. the conv before it; a paste of no boxes points the tap at the executor the detect ran in).

Before se_plan was planned per image, measured on an MI355X: D0 at 128^2 differed at B = 8 from the projection conv
of blocks_12 on (the 1152-channel SE's scale; max |d| 8.9e-8, 1.4e-7 of the tensor's largest value) and at B = 16
from blocks_9 on (the 672-channel SE), ending in 1018 of 3069 scores (up to 2.2e-7) and 11061 of 12276 box
coordinates (up to 5.5e-4 px); D4 at 256^2 differed at B = 4 from blocks_31 on, 1856 of 12276 scores (up to 2.2e-8)
and 34009 of 49104 box coordinates (up to 4.3e-4 px); B = 4 of D0 at either size was equal.  The module takes 3 s.
"""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(96, 160), (60, 97), (200, 75), (128, 128), (37, 23), (300, 411), (64, 512), (511, 90)]


def _frames(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, SIZES[i % len(SIZES)] + (3,), dtype=np.uint8) for i in range(n)]


class Served:
    """One Detector, its frames preprocessed once, and every frame's single-image results."""

    def __init__(self, model, S, nframes, gamma=(0.5, 1.5)):
        from mladversarialobjectdetection_amd import _lib
        from mladversarialobjectdetection_amd import weights as W
        from mladversarialobjectdetection_amd.detector import Detector
        blob = W.synthetic_blob(_lib.Context(model, S, 1).manifest(), seed=0, person_bias=2.0, gamma=gamma)
        self.det = Detector(params={"image_size": S, "nms_configs": {"score_thresh": 0.0}}, model=model,
                            weights=blob, max_batch=nframes, rng_seed=5)
        self.drv, self.v = self.det.driver, self.det.driver.model
        self.frames = _frames(nframes, 21)
        self.images, _ = self.drv._preprocess(self.frames)
        self.single_detect = [self.detect([i])[0] for i in range(nframes)]
        self.single_serve = [self.serve([i])[0] for i in range(nframes)]
        self._att = None
        # a network that computes something: finite boxes and scores that vary over the anchors
        for sc, _, bx in self.single_detect:
            assert np.isfinite(bx).all() and np.isfinite(sc).all() and sc.std() > 1e-4, (model, S, sc.std())

    def detect(self, idx):
        """-> per image of the call (scores, classes, boxes) as numpy."""
        bx, sc, cl = self.v.detect(self.images[torch.as_tensor(idx, device=self.images.device)])
        torch.cuda.synchronize()
        bx, sc, cl = bx.cpu().numpy(), sc.cpu().numpy(), cl.cpu().numpy()
        return [(sc[k], cl[k], bx[k]) for k in range(len(idx))]

    def serve(self, idx):
        out = [t.cpu().numpy() for t in self.drv.serve([self.frames[i] for i in idx])]
        return [tuple(o[k] for o in out) for k in range(len(idx))]

    # ---- diagnosis ------------------------------------------------------------------------------------
    def _taps(self, idx):
        """{BN name: its input [B, ...] after a detect of images idx} through phx_debug_tap."""
        from mladversarialobjectdetection_amd._lib import PhxError
        from mladversarialobjectdetection_amd.attacker import PatchAttacker, Patcher
        # phx_debug_tap reads the executor of the last step-like call: a paste of no boxes at this batch size
        # points it at the executor the detect below runs in
        if self._att is None:
            self._att = PatchAttacker(self.v, seed=7)
        Patcher(self._att)(([np.zeros((0, 4), np.float32)] * len(idx),
                            self.images[torch.as_tensor(idx, device=self.images.device)]), step=0)
        self.detect(idx)
        st = torch.cuda.current_stream().cuda_stream
        names = [m["name"][:-len("/moving_mean")] for m in self.v.manifest if m["name"].endswith("/moving_mean")]
        out = {}
        for name in names:
            probe = torch.empty(1, device="cuda")
            try:
                self.v.ctx.call("phx_debug_tap", name.encode(), 0, probe.data_ptr(), 1, st)
                n = 1
            except PhxError as e:
                m = re.search(r"the tensor has (\d+) elements", str(e))
                if not m:
                    continue
                n = int(m.group(1))
            buf = torch.empty(n, device="cuda")
            try:
                self.v.ctx.call("phx_debug_tap", name.encode(), 0, buf.data_ptr(), n, st)
            except PhxError:
                continue
            out[name] = buf.cpu().numpy().reshape(len(idx), -1)
        return out

    def first_differing_op(self, idx, k):
        """The first op (in weight order) whose tensor differs for image idx[k] between the batch and alone."""
        try:
            alone, batch = self._taps([idx[k]]), self._taps(idx)
            for name, a in alone.items():
                b = batch.get(name)
                if b is not None and not _same(a[0], b[k]):
                    d = np.abs(a[0].astype(np.float64) - b[k])
                    rel = d.max() / max(np.abs(a[0]).max(), 1e-30)
                    return f"first differing op: the conv before {name}: max |d| {d.max():.3e} ({rel:.1e} of max |x|)"
            return f"no tapped tensor differs ({len(alone)} tapped)"
        except Exception as e:  # the diagnosis must not hide the finding
            return f"(no per-op diagnosis: {e})"


_CACHE = {}


def _served(model, S, n, **kw):
    if (model, S) not in _CACHE:
        _CACHE.clear()  # one context at a time
        _CACHE[(model, S)] = Served(model, S, n, **kw)
    return _CACHE[(model, S)]


def _same(a, b):
    """Bit for bit (a NaN equals itself)."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _compare(s, idx):
    names_d, names_s = ("scores", "classes", "boxes"), ("boxes", "scores", "classes", "valid_len")
    det, srv = s.detect(idx), s.serve(idx)
    bad = []
    for k, i in enumerate(idx):
        for nm, got, want in zip(names_d, det[k], s.single_detect[i]):
            if not _same(got, want):
                d = np.abs(got.astype(np.float64) - want.astype(np.float64))
                bad.append(f"detect {nm}, image {i} at position {k} of {len(idx)}: {int((got != want).sum())} of "
                           f"{got.size} differ, max |d| {np.nanmax(d):.3e}")
        for nm, got, want in zip(names_s, srv[k], s.single_serve[i]):
            if not _same(got, want):
                bad.append(f"serve {nm}, image {i} at position {k} of {len(idx)} differs")
        if bad:
            bad.append(s.first_differing_op(idx, k))
            break
    assert not bad, "\n".join(bad)
    assert all(int(srv[k][3]) == 100 for k in range(len(idx)))  # score_thresh 0.0: every row is a detection


ORDER2 = [11, 3, 14, 0, 7, 12, 5, 9, 1, 15, 6, 10, 2, 13, 8, 4]


@pytest.mark.parametrize("idx", [list(range(4)), list(range(8)), list(range(16)), ORDER2, [5, 9, 2, 12, 7, 0, 15, 3]],
                         ids=["b4", "b8", "b16", "b16_reordered", "b8_reordered"])
def test_d0_128_batches_equal_single_frames(idx):
    _compare(_served("efficientdet-d0", 128, 16), idx)


def test_d0_512_batch_equals_single_frames():
    s = _served("efficientdet-d0", 512, 4)
    _compare(s, [0, 1, 2, 3])
    _compare(s, [2, 0, 3, 1])


def test_d4_256_batch_equals_single_frames():
    # (with the default BN scales, uniform in (0.5, 1.5), D4's inference-mode activations overflow: every score
    # is 1 and 38 % of the boxes are not finite; (0.4, 1.0) keeps scores in 0.05 .. 0.09 and boxes finite)
    s = _served("efficientdet-d4", 256, 4, gamma=(0.4, 1.0))
    _compare(s, [0, 1, 2, 3])
    _compare(s, [3, 2, 1])
    _CACHE.clear()
