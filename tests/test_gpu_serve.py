"""GPU: serving raw uint8 frames — phx_serve_preprocess, phx_nms_global, phx_serve and the Detector
mirror — against the restatement in tests/serve_oracle.py and the fp64 oracle.

The victim is D0 at 128^2 (3069 anchors) with the synthetic weights at the reference's -log(99)
class prior, and the class-predict bias lifted by 4.0 for class 0 (person) on anchor slots 0-4 and for
class 16 on slots 5-8, so two classes pass the 0.5 threshold.  On the fp64 restatement the frames
below give 24-26 candidates per image and 3 selections (1 person, 2 of class 17), and no anchor's
score is closer than 1.8e-4 to 0.5 (the fp32-vs-fp64 score difference is ~1e-6), so candidate sets
and selection order are unambiguous.

Measured on an MI355X, max |device - preprocess64| per frame against the derived bound (the tests
print each figure before asserting it): 7.6e-8 ... 3.8e-7 against 1.6e-6 ... 7.6e-6; the forward's
scores 1.6e-7 from the fp64 oracle's against 2e-5.
"""
import numpy as np
import pytest
import torch

import serve_oracle as so

pytestmark = pytest.mark.gpu

S = 128
SHAPES = [(96, 160), (60, 97), (200, 75), (128, 128)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _frames(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _mean_std(fam="efficientdet"):
    from mladversarialobjectdetection_amd.attacker import MEAN_RGB, STDDEV_RGB
    return MEAN_RGB[fam], STDDEV_RGB[fam]


def _preprocess(ctx, frames):
    """phx_serve_preprocess on a bare context (it needs no weights)."""
    from mladversarialobjectdetection_amd.detector import pack_frames
    p = pack_frames(frames, torch.device("cuda", 0))
    B = len(p.offsets)
    images = torch.full((B, ctx.image_size, ctx.image_size, 3), 7.0, device="cuda")  # the kernel writes the padding
    scales = torch.empty(B, device="cuda")
    ctx.call("phx_serve_preprocess", p.src.data_ptr(), p.offsets.ctypes.data, p.dims.ctypes.data, B,
             images.data_ptr(), scales.data_ptr(), _stream())
    torch.cuda.synchronize()
    return images.cpu().numpy(), scales.cpu().numpy()


def _check_preprocess(images, scales, frames, mean, std):
    worst = 0.0
    for b, fr in enumerate(frames):
        h, w, _ = fr.shape
        sh, sw, _ = so.dims(h, w, S)
        ref = so.preprocess64(fr, S, mean, std)
        ty, tx = so.taps(h, w, S)
        # one rounding per tap and per weight of each pass, non-negative weights summing to 1, + 8 for
        # the normalisation, the weight normalisation and the row buffer; 2.65 bounds |normalised value|
        bound = (ty + tx + 8) * 2.0 ** -24 * 2.65
        err = np.abs(images[b].astype(np.float64) - ref).max()
        print(f"preprocess {h}x{w} -> {sh}x{sw}: taps ({ty}, {tx}) max |d| {err:.3e} bound {bound:.3e}")
        assert np.abs(ref).max() <= 2.65
        assert err <= bound, (fr.shape, err, bound)
        worst = max(worst, err / bound)
        assert np.array_equal(images[b, sh:], np.zeros_like(images[b, sh:]))
        assert np.array_equal(images[b, :, sw:], np.zeros_like(images[b, :, sw:]))
        assert scales[b] == so.scale_to_original(h, w, S)
    return worst


def test_preprocess_matches_fp64():
    """One packed call over six frames of different sizes: up- and downscales on either axis, the
    identity, the fp32 truncation case (60 x 97 -> 79 x 127) and 720p (22 taps per axis)."""
    from mladversarialobjectdetection_amd import _lib
    shapes = SHAPES + [(37, 23), (720, 1280)]
    frames = _frames(shapes, 2)
    ctx = _lib.Context("efficientdet-d0", image_size=S, max_batch=6)
    images, scales = _preprocess(ctx, frames)
    _check_preprocess(images, scales, frames, *_mean_std())
    # 97 * fp32(128 / 97) = 127.99999 truncates to 127: column 127 is padding, column 126 is image
    assert not images[1, :, 127].any() and images[1, :79, 126].any()
    # a frame already S x S is exactly the normalised frame
    mean, std = (np.asarray(v, np.float32) for v in _mean_std())
    np.testing.assert_array_equal(images[3], ((frames[3].astype(np.float32) - mean) / std).astype(np.float32))


def test_preprocess_lite_constants():
    from mladversarialobjectdetection_amd import _lib
    frames = _frames([(50, 211)], 4)
    ctx = _lib.Context("efficientdet-lite0", image_size=S, max_batch=1)
    images, scales = _preprocess(ctx, frames)
    _check_preprocess(images, scales, frames, *_mean_std("lite"))


# ---- phx_nms_global on synthetic candidates -------------------------------------------------------
@pytest.fixture(scope="module")
def serving():
    """The frozen-BN victim, its frames and everything the library computes for them, once."""
    from mladversarialobjectdetection_amd import weights as W
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.detector import Detector
    man = _lib.Context("efficientdet-d0", image_size=S).manifest()
    blob = W.synthetic_blob(man, seed=0, person_bias=0.0)
    e = [m for m in man if m["name"] == "class_net/class-predict/bias"][0]
    bias = blob[e["offset"]:e["offset"] + 810].reshape(9, 90)
    bias[0:5, 0] += 4.0
    bias[5:9, 16] += 4.0
    det = Detector(params={"image_size": S, "nms_configs": {"score_thresh": 0.5}}, model="efficientdet-d0",
                   weights=blob, max_batch=4, rng_seed=5)
    frames = _frames(SHAPES, 6)
    drv = det.driver
    images, scales = drv._preprocess(frames)
    boxes, scores, classes = drv.model.detect(images)
    out = drv.serve(frames)
    torch.cuda.synchronize()
    return dict(det=det, drv=drv, blob=blob, frames=frames, images=images.cpu().numpy(), scales=scales.cpu().numpy(),
                boxes=boxes.cpu().numpy(), scores=scores.cpu().numpy(), classes=classes.cpu().numpy(),
                out=[t.cpu().numpy() for t in out])


@pytest.mark.parametrize("score_thresh", [0.5, 0.0])
def test_nms_global_matches_restatement(serving, score_thresh):
    """test_soft_nms_exact's candidates with classes and per-image scales."""
    drv = serving["drv"]
    rng = np.random.default_rng(3)
    B, N = 3, 400
    yx = rng.uniform(0, 100, (B, N, 2))
    hw = rng.uniform(8, 40, (B, N, 2))
    bx = np.concatenate([yx, yx + hw], -1).astype(np.float32)
    sc = rng.uniform(0.3, 1.0, (B, N)).astype(np.float32)
    cl = rng.integers(0, 90, (B, N)).astype(np.int32)
    cnt = np.array([N, 250, 0], np.int32)
    scales = np.array([1.25, 0.7578125, 1.0], np.float32)
    nt = 0.001 if score_thresh == 0.0 else score_thresh
    dev = [torch.as_tensor(a).cuda() for a in (bx, sc, cl, cnt, scales)]
    drv.model.ctx.set_score_thresh(score_thresh)
    try:
        scaled = [t.cpu().numpy() for t in drv.postprocess_global(*dev)]
        plain = [t.cpu().numpy() for t in drv.postprocess_global(*dev[:4], scales=None)]
    finally:
        drv.model.ctx.set_score_thresh(0.5)
    for b in range(B):
        for got, scale in ((scaled, scales[b]), (plain, None)):  # null scales: boxes stay in model pixels
            rb, rs, rc, n = so.postprocess_global(bx[b, :cnt[b]], sc[b, :cnt[b]], cl[b, :cnt[b]], S, nt, scale)
            ob, os_, oc, on = (g[b] for g in got)
            assert on == n
            np.testing.assert_array_equal(ob, rb)
            np.testing.assert_array_equal(oc, rc)
            # decayed scores carry the device expf (1 ulp) of the gaussian decay factors
            np.testing.assert_allclose(os_[:n], rs[:n], rtol=2e-6, atol=0)
            assert not ob[n:].any() and not os_[n:].any() and not oc[n:].any()
        if score_thresh == 0.0 and cnt[b] > 100:
            assert scaled[3][b] == 100  # truncated at max_output_size
    assert scaled[3][2] == 0


# ---- phx_serve --------------------------------------------------------------------------------------
def test_serve_equals_the_composition(serving):
    """serve == postprocess_global over the library's own detect(_preprocess(frames)) fp32 outputs:
    the candidate mode without masks, the selected-index output, the class gather, clip then scale."""
    ob, os_, oc, on = serving["out"]
    sc, cl, bx = serving["scores"], serving["classes"], serving["boxes"]
    nsel, seen = 0, set()
    for b, fr in enumerate(serving["frames"]):
        assert (sc[b] > 0.5).sum() >= 20  # the inputs produce real candidates
        scale = so.scale_to_original(fr.shape[0], fr.shape[1], S)
        assert serving["scales"][b] == scale
        rb, rs, rc, n = so.postprocess_global(bx[b], sc[b], cl[b], S, 0.5, scale)
        nsel += n
        seen |= set(rc[:n].tolist())
        assert on[b] == n
        np.testing.assert_array_equal(ob[b], rb)
        np.testing.assert_array_equal(oc[b], rc)
        np.testing.assert_allclose(os_[b], rs, rtol=2e-6, atol=0)
    assert nsel >= 3 and {1.0, 17.0} <= seen


def test_serve_matches_fp64_oracle(serving):
    """The preprocess and the inference-mode forward against the fp64 oracle on preprocess64's images
    (the bounds of test_frozen_bn_detect_matches_oracle, the same forward)."""
    from mladversarialobjectdetection_amd import weights as W
    from oracle import detector as D
    mean, std = _mean_std()
    ref = np.stack([so.preprocess64(fr, S, mean, std) for fr in serving["frames"]])
    det = D.Detector(W.unpack(serving["drv"].model.manifest, serving["blob"].copy()), "efficientdet-d0", S,
                     training=False)
    with torch.no_grad():
        rs, rc, rb = D.pre_nms(*det(torch.as_tensor(ref)), S)
    d = np.abs(serving["scores"] - rs.numpy()).max()
    agree = (serving["classes"] == rc.numpy()).mean()
    print(f"serve forward vs fp64: max |d score| {d:.3e}, class agreement {agree:.5f}")
    assert d <= 2e-5
    assert agree >= 0.999


# ---- Detector ---------------------------------------------------------------------------------------
def test_detector_infer(serving):
    det, drv, frames = serving["det"], serving["drv"], serving["frames"]
    per_frame = []
    for fr in frames:
        ob, os_, oc, on = (t.cpu().numpy()[0] for t in drv.serve([fr]))
        rows = [i for i in range(int(on)) if oc[i] == 1]
        bb, sc = det.infer(fr)
        assert isinstance(bb, list) and isinstance(sc, list)
        assert bb == [tuple(ob[i].tolist()) for i in rows] and all(isinstance(x, tuple) and len(x) == 4 for x in bb)
        assert sc == [os_[i] for i in rows]
        h, w = fr.shape[:2]
        scale = float(so.scale_to_original(h, w, S))
        assert all(0.0 <= v <= S * scale for x in bb for v in x)  # frame pixels
        per_frame.append((bb, sc))
    assert sum(len(bb) for bb, _ in per_frame) >= 1
    k = max(range(len(frames)), key=lambda i: len(per_frame[i][0]))
    bb1, sc1 = det.infer(frames[k], max_boxes=1)
    assert bb1 == per_frame[k][0][:1] and sc1 == per_frame[k][1][:1]
    # infer_batch of one frame is infer
    assert det.infer_batch([frames[k]]) == [per_frame[k]]


def test_infer_batch_equals_per_frame_infer(serving):
    """infer_batch (one phx_serve call at B = 4) against infer per frame (B = 1), array_equal: an
    executor planned for inference BN chooses every summation order per image (gemm_plan_images:
    the GEMM kernel by one image's rows, the SE pools' chunks for a fixed image count), so an image's
    detections do not depend on the batch it was served in.  (Planned by the batch's row count, the
    boxes differed by up to 4.6e-5 px between the two batch sizes.)"""
    det, frames = serving["det"], serving["frames"]
    per_frame = [det.infer(fr) for fr in frames]
    batch = det.infer_batch(frames)
    assert len(batch) == len(frames)
    for i, ((bb, sc), (rb, rs)) in enumerate(zip(batch, per_frame)):
        assert len(bb) == len(rb) and len(sc) == len(rs)
        if bb:
            db = np.abs(np.asarray(bb, np.float64) - np.asarray(rb, np.float64)).max()
            ds = np.abs(np.asarray(sc, np.float64) - np.asarray(rs, np.float64)).max()
            print(f"infer_batch vs infer, frame {i}: {len(bb)} person box(es), max |d box| {db:.3e} px, max |d score| {ds:.3e}")
    for (bb, sc), (rb, rs) in zip(batch, per_frame):
        np.testing.assert_array_equal(np.asarray(bb, np.float32).reshape(-1, 4), np.asarray(rb, np.float32).reshape(-1, 4))
        np.testing.assert_array_equal(np.asarray(sc, np.float32), np.asarray(rs, np.float32))


def test_detector_score_thresh_zero(serving):
    drv, frames = serving["drv"], serving["frames"]
    drv.model.config.override({"nms_configs": {"score_thresh": 0.0}})
    try:
        ob, os_, oc, on = (t.cpu().numpy() for t in drv.serve(frames))
    finally:
        drv.model.config.override({"nms_configs": {"score_thresh": 0.5}})
    for b, fr in enumerate(frames):
        assert on[b] == 100
        assert (np.diff(os_[b]) <= 0).all() and os_[b, -1] > 0.001
        hi = np.float32(S) * so.scale_to_original(fr.shape[0], fr.shape[1], S)
        assert ob[b].min() >= 0 and ob[b].max() <= hi
        assert oc[b].min() >= 1 and oc[b].max() <= 90


def test_serve_is_inference_mode_whatever_bn_mode(serving):
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    from mladversarialobjectdetection_amd.detector import ServeDriver
    v = EfficientDetVictim("efficientdet-d0", serving["blob"], image_size=S, max_batch=4, rng_seed=5, bn_mode="local",
                           score_thresh=0.5)
    out = ServeDriver(v).serve(serving["frames"])
    for got, want in zip(out, serving["out"]):
        assert torch.equal(got.cpu(), torch.as_tensor(want))
    np.testing.assert_array_equal(v.read_weights(), serving["blob"])  # no moving-statistics update


def test_serve_workspace_is_reserved_once(serving):
    """The first call of a batch size reserves the canvas; later calls allocate nothing more."""
    drv, frames = serving["drv"], serving["frames"]
    ws = drv.model.ctx.workspace_bytes(4)
    assert ws >= 4 * S * S * 3 * 4  # the preprocessed batch is part of the reported workspace
    for _ in range(10):  # more calls than the frame-table ring has slots
        out = drv.serve(frames)
    assert drv.model.ctx.workspace_bytes(4) == ws
    for got, want in zip(out, serving["out"]):
        assert torch.equal(got.cpu(), torch.as_tensor(want))  # and the calls repeat bit for bit


def test_serve_is_refused_while_a_prefetch_is_pending(serving):
    """phx_set_next leaves the next batch's first pass running on a library stream: phx_serve returns
    PHX_ESTATE until the step that consumes it has been issued or the prefetch is withdrawn."""
    from mladversarialobjectdetection_amd._lib import PhxError
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim, PatchAttacker
    from mladversarialobjectdetection_amd.detector import ServeDriver
    v = EfficientDetVictim("efficientdet-d0", serving["blob"], image_size=S, max_batch=2, rng_seed=5, bn_mode="local",
                           score_thresh=0.5)
    att = PatchAttacker(v, seed=7)
    imgs = [torch.as_tensor(np.random.default_rng(s).uniform(-1, 1, (2, S, S, 3)).astype(np.float32)).cuda()
            for s in (1, 2)]
    att.train_step(imgs[0], next_inputs=imgs[1])
    drv = ServeDriver(v)
    with pytest.raises(PhxError, match="prefetch"):
        drv.serve(serving["frames"][:2])
    v.ctx.call("phx_set_next", None, 0, 0)  # withdrawn
    ob, os_, oc, on = drv.serve(serving["frames"][:2])
    torch.cuda.synchronize()
    assert int(on.min()) >= 0 and torch.isfinite(ob).all()


def test_filter_by_thresh(serving):
    from mladversarialobjectdetection_amd.detector import filter_by_thresh
    bb, sc = serving["det"].infer(serving["frames"][0])
    t = sc[0] if sc else 0.5
    fb, fs = filter_by_thresh(bb + [(0, 0, 1, 1)], sc + [np.float32(0.25)], t)
    assert fs == [s for s in sc if s >= t] and len(fb) == len(fs) and (not sc or sc[0] in fs)  # keeps >=
