"""GPU: phx_persons (the person rows of phx_serve's device outputs: detector.py:48-57, then
util.filter_by_thresh, util.py:163-174, and demo.py:81's max(sc)) on injected serve outputs against a
numpy restatement, exact match.  B = 3, one call covers: rows that mix classes, scores on both sides
of the threshold and exactly at float32(thresh), persons only below the threshold (count 0, best > 0),
valid = 0, valid = 100 with kept rows in both 64-row passes, and garbage beyond valid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THRESH = 0.55
N = 100


def _restate(boxes, scores, classes, valid, thresh):
    pb, pc, best = np.zeros_like(boxes), np.zeros(len(valid), np.int32), np.zeros(len(valid), np.float32)
    for b, n in enumerate(valid):
        person = classes[b, :n] == 1
        keep = person & (scores[b, :n] >= np.float32(thresh))
        pc[b] = keep.sum()
        pb[b, :pc[b]] = boxes[b, :n][keep]
        best[b] = scores[b, :n][person].max() if person.any() else 0
    return pb, pc, best


def _inputs():
    rng = np.random.default_rng(31)
    boxes = rng.uniform(0, 500, (3, N, 4)).astype(np.float32)
    scores = rng.uniform(0.0, 1.0, (3, N)).astype(np.float32)
    classes = rng.integers(1, 4, (3, N)).astype(np.float32)  # 1 = person, 2 and 3 are not
    t = np.float32(THRESH)
    # frame 0: every row valid; rows exactly at, one ulp below and one ulp above float32(thresh), in both
    # halves; a non-person with the highest score; the last row a kept person
    classes[0, [3, 4, 5, 70, 71, 72, 99]] = 1
    scores[0, [3, 70]] = t
    scores[0, [4, 71]] = np.nextafter(t, np.float32(0))
    scores[0, [5, 72]] = np.nextafter(t, np.float32(1))
    scores[0, 99] = 0.9
    classes[0, 10], scores[0, 10] = 2, 1.0
    # frame 1: valid = 0, persons far above the threshold everywhere
    classes[1], scores[1] = 1, 0.99
    # frame 2: valid = 37, its persons all below the threshold; beyond valid persons above it, a NaN and an inf
    scores[2, :37] = rng.uniform(0.0, 0.5, 37).astype(np.float32)
    classes[2, [0, 7, 36]] = 1
    classes[2, 37:], scores[2, 37:] = 1, 0.95
    scores[2, 40], scores[2, 41] = np.nan, np.inf
    boxes[2, 50:] = np.nan
    valid = np.asarray([100, 0, 37], np.int32)
    return boxes, scores, classes, valid


def test_persons_matches_numpy_restatement():
    from mladversarialobjectdetection_amd import _lib
    ctx = _lib.Context("efficientdet-d0", 0, 1)
    boxes, scores, classes, valid = _inputs()
    want_b, want_c, want_s = _restate(boxes, scores, classes, valid, THRESH)
    # the cases are there: kept rows in both passes, a frame with persons only below the threshold
    keep0 = (classes[0] == 1) & (scores[0] >= np.float32(THRESH))
    assert keep0[:64].any() and keep0[64:].any() and keep0[3] and keep0[70] and not keep0[4] and not keep0[71]
    assert want_c.tolist()[1:] == [0, 0] and want_s[1] == 0 and 0 < want_s[2] < THRESH and want_c[0] > 10
    dev = torch.device("cuda", 0)
    d = [torch.as_tensor(a, device=dev) for a in (boxes, scores, classes, valid)]
    # outputs between guard words
    G = 16
    pb = torch.full((3 * N * 4 + 2 * G,), -7.0, device=dev)
    pc = torch.full((3 + 2 * G,), -7, dtype=torch.int32, device=dev)
    best = torch.full((3 + 2 * G,), -7.0, device=dev)
    ctx.call("phx_persons", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 3, THRESH,
             pb[G:].data_ptr(), pc[G:].data_ptr(), best[G:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pb, pc, best = pb.cpu().numpy(), pc.cpu().numpy(), best.cpu().numpy()
    for a in (pb, pc, best):
        assert (a[:G] == -7).all() and (a[-G:] == -7).all()
    got_b, got_c, got_s = pb[G:-G].reshape(3, N, 4), pc[G:-G], best[G:-G]
    print(f"persons: counts {got_c.tolist()} (want {want_c.tolist()}), best {got_s.tolist()} (want {want_s.tolist()})")
    np.testing.assert_array_equal(got_c, want_c)
    assert got_s.tobytes() == want_s.tobytes()
    assert got_b.tobytes() == want_b.tobytes()
    # the inputs are untouched
    for t, a in zip(d, (boxes, scores, classes, valid)):
        assert t.cpu().numpy().tobytes() == a.tobytes()


def test_persons_refusals():
    from mladversarialobjectdetection_amd import _lib
    ctx = _lib.Context("efficientdet-d0", 0, 1)
    t = torch.zeros(N * 4 + 4, device="cuda")
    i = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = lambda boxes, pboxes, B=1: (boxes, t.data_ptr(), t.data_ptr(), i.data_ptr(), B, THRESH, pboxes, i.data_ptr(),
                                       t.data_ptr(), None)
    o = torch.zeros(N * 4 + 4, device="cuda")
    for bad, match in ((args(t.data_ptr(), o.data_ptr(), 0), "B must be >= 1"), (args(None, o.data_ptr()), "null"),
                       (args(t.data_ptr() + 4, o.data_ptr()), "16-byte aligned"),
                       (args(t.data_ptr(), t.data_ptr()), "alias")):
        with pytest.raises(_lib.PhxError, match=match):
            ctx.call("phx_persons", *bad)
