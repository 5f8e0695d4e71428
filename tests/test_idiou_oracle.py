"""tests/idiou_oracle.py (the fp64 restatement of regression_loss.py's InverseDIOULoss) against hand-computed
pairs, a loop-for-loop numpy transcription, central differences, and the tie / kink gradient rules."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import idiou_oracle as IO

T = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731


def pair(g, p):
    return float(IO.idiou_pairs(T([g]), T([p]))[0, 0])


# gt, pred, 1 - diou_loss worked by hand from regression_loss.py:101-142
HAND = [
    # identical: iou 1, "centres" equal, diou = 1
    ([0, 0, 10, 10], [0, 0, 10, 10], 1.0),
    # disjoint: iou 0; far corners (10,10) and (30,30): dist 800; enclosure 30 x 30: diag 1800
    ([0, 0, 10, 10], [20, 20, 30, 30], -800.0 / 1800.0),
    # zero-area pred inside the gt: iou 0 / 100; corners (10,10), (5,5): dist 50; enclosure 10 x 10
    ([0, 0, 10, 10], [5, 5, 5, 5], -50.0 / 200.0),
    # gt with ymax < ymin: height -10, area -100 (unclamped, :45-47); union -100 + 100 - 0 = 0 -> iou 0 by
    # divide_no_nan; gt "centre" (10 - 10, 0 + 10) = (0, 10), pred's (10, 10): dist 100; enclosure 10 x 10
    ([10, 0, 0, 10], [0, 0, 10, 10], -100.0 / 200.0),
    # both a point: both divide_no_nan denominators are 0
    ([3, 4, 3, 4], [3, 4, 3, 4], 0.0),
]


@pytest.mark.parametrize("g,p,want", HAND)
def test_hand_computed_pairs(g, p, want):
    assert pair(g, p) == pytest.approx(want, abs=1e-15)
    assert IO.idiou_loops([g], [p]) == pytest.approx(want + IO.EPS, abs=1e-15)


def _random_sets(rng, G, P, flip=True):
    def boxes(n):
        a = rng.uniform(0, 100, (n, 2))
        s = rng.uniform(-5 if flip else 2, 60, (n, 2))  # (some flipped / negative extents)
        return np.concatenate([a, a + s], -1)
    return boxes(G), boxes(P)


def test_matches_loop_transcription():
    rng = np.random.default_rng(0)
    for G, P in [(1, 1), (3, 17), (7, 5), (100, 40), (4, 0), (0, 6)]:
        gt, pred = _random_sets(rng, G, P)
        a = float(IO.idiou_image(T(gt), T(pred).reshape(-1, 4)))
        assert a == pytest.approx(IO.idiou_loops(gt, pred), rel=1e-13, abs=1e-13)
    # degenerate members beside ordinary ones
    gt = np.array([[0, 0, 10, 10], [10, 0, 0, 10], [3, 4, 3, 4]], np.float64)
    pred = np.array([[5, 5, 5, 5], [3, 4, 3, 4], [1, 1, 9, 9]], np.float64)
    assert float(IO.idiou_image(T(gt), T(pred))) == pytest.approx(IO.idiou_loops(gt, pred), abs=1e-14)


def test_batch_is_sum_over_images():
    rng = np.random.default_rng(1)
    sets = [_random_sets(rng, 3, 9), _random_sets(rng, 2, 0), _random_sets(rng, 0, 4)]
    v = IO.idiou_batch([T(g) for g, _ in sets], [T(p).reshape(-1, 4) for _, p in sets])
    assert float(v) == pytest.approx(sum(IO.idiou_loops(g, p) for g, p in sets), abs=1e-13)


def test_autograd_matches_central_differences():
    """Away from kinks: random boxes in general position (no equal coordinates, a clear best pred per gt)."""
    rng = np.random.default_rng(2)
    gt, pred = _random_sets(rng, 5, 12, flip=False)
    pairs = IO.idiou_pairs(T(gt), T(pred)).numpy()
    top = np.sort(pairs, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 1e-3  # the argmax cannot move within the step below
    p = T(pred).requires_grad_(True)
    IO.idiou_image(T(gt), p).backward()
    g = p.grad.numpy()
    h = 1e-6
    num = np.zeros_like(pred)
    for i in range(pred.shape[0]):
        for j in range(4):
            a, b = pred.copy(), pred.copy()
            a[i, j] += h
            b[i, j] -= h
            num[i, j] = (IO.idiou_loops(gt, a) - IO.idiou_loops(gt, b)) / (2 * h)
    assert np.abs(g).max() > 1e-3
    np.testing.assert_allclose(g, num, rtol=1e-6, atol=1e-8)


def _grad(gt, pred):
    p = T(pred).requires_grad_(True)
    IO.idiou_image(T(gt), p).backward()
    return p.grad.numpy()


def test_reduce_max_splits_exact_ties_equally():
    gt = [[0, 0, 10, 10]]
    one = [[1, 2, 8, 9], [50, 50, 60, 60]]
    dup = [[1, 2, 8, 9], [50, 50, 60, 60], [1, 2, 8, 9], [1, 2, 8, 9]]
    g1, g3 = _grad(gt, one), _grad(gt, dup)
    assert np.abs(g1[0]).min() > 0
    for k in (0, 2, 3):
        np.testing.assert_allclose(g3[k], g1[0] / 3.0, rtol=1e-15)
    assert not g3[1].any() and not g1[1].any()
    # the value does not change with the copies
    assert float(IO.idiou_image(T(gt), T(one))) == float(IO.idiou_image(T(gt), T(dup)))


def test_maximum_minimum_ties_go_to_the_gt():
    """tf.maximum(x, y) / tf.minimum(x, y) at x == y: x (the gt) takes the gradient.  A pred that shares all
    four coordinates with its gt gets gradient through its own clamped height / width only: the intersection
    and enclosure corners all route to the gt."""
    x = T([2.0]).requires_grad_(True)
    y = T([2.0]).requires_grad_(True)
    (IO.tf_max(x, y) + 10 * IO.tf_min(x, y)).sum().backward()
    assert x.grad.item() == 11.0 and y.grad.item() == 0.0
    g = np.array([0.0, 0.0, 10.0, 10.0])
    got = _grad([g], [g])[0]
    # identical boxes: ia = pa = ga = ua = 100, iou = pa-term only: d iou / d pa = -ia / ua^2 = -1/100;
    # pa = pw ph: d / d ph = -10/100 = -0.1; the centre term's derivative is 0 (dist = 0).  ph = ymax - ymin.
    np.testing.assert_allclose(got, [0.1, 0.1, -0.1, -0.1], rtol=1e-14)


def test_clamp_at_zero_passes_only_positive():
    """maximum(0., v): v = 0 gets no gradient (the tie goes to the constant), v < 0 none, v > 0 all."""
    for v, want in ((0.0, 0.0), (-1.0, 0.0), (1.0, 1.0)):
        t = T([v]).requires_grad_(True)
        IO.tf_max(torch.zeros((), dtype=torch.float64), t).sum().backward()
        assert t.grad.item() == want
    # a zero-height pred: its ymax / ymin get gradient from the corners that win strictly only, none
    # through the clamped height.  gt [0,0,10,10], pred [5,2,5,8]: iy0 = max(0,5) -> pred, iy1 = min(10,5)
    # -> pred, but ih = max(0, 0) passes nothing; enclosure corners are the gt's; the centre term reaches ymin
    # through p.ymin + ph only by its first summand.
    g, p = [0.0, 0.0, 10.0, 10.0], [5.0, 2.0, 5.0, 8.0]
    got = _grad([g], [p])[0]
    # dist = (10 - 5)^2 + (10 - 8)^2, diag = 200: d(-dist/diag)/d ymin = 2 * 5 / 200; xmin and xmax: the
    # centre's x is xmin + pw = xmax: d / d xmin = 0 net (+ via xmin, - via pw), d / d xmax = 2 * 2 / 200;
    # iou = 0 / 100 with d iou / d ia = 1/100: ia = iw * ih, ih = 0: d / d iw = 0, d / d ih = iw / 100 but the
    # clamp blocks it
    np.testing.assert_allclose(got, [0.05, 0.0, 0.0, 0.02], rtol=1e-14, atol=1e-17)


def test_divide_no_nan_has_zero_gradient_at_zero_denominator():
    x = T([3.0, 3.0]).requires_grad_(True)
    y = T([0.0, 2.0]).requires_grad_(True)
    IO.div_no_nan(x, y).sum().backward()
    assert x.grad.tolist() == [0.0, 0.5] and y.grad.tolist() == [0.0, -0.75]
    # both boxes a point: the value is 0 and nothing flows
    got = _grad([[3.0, 4.0, 3.0, 4.0]], [[3.0, 4.0, 3.0, 4.0]])
    assert not got.any() and np.isfinite(got).all()


def test_no_gt_or_no_pred_gives_epsilon_and_zero_gradient():
    pred = T([[1.0, 2.0, 8.0, 9.0]]).requires_grad_(True)
    v = IO.idiou_image(T(np.zeros((0, 4))), pred)
    assert float(v.detach()) == IO.EPS
    v.backward()
    assert not pred.grad.numpy().any()
    empty = T(np.zeros((0, 4))).requires_grad_(True)
    v = IO.idiou_image(T([[0.0, 0.0, 10.0, 10.0]]), empty)
    assert float(v.detach()) == IO.EPS
    v.backward()
    assert empty.grad.shape == (0, 4)
    assert float(IO.idiou_batch([T(np.zeros((0, 4)))] * 3, [empty] * 3)) == pytest.approx(3 * IO.EPS, abs=0)
    assert IO.idiou_loops(np.zeros((0, 4)), [[1, 2, 8, 9]]) == IO.EPS
    assert IO.idiou_loops([[0, 0, 10, 10]], np.zeros((0, 4))) == IO.EPS


def test_decode_matches_pre_nms_and_carries_gradient():
    """decode() equals oracle.detector.pre_nms's boxes and, unlike them, is differentiable."""
    from oracle import detector as D
    rng = np.random.default_rng(3)
    S = 64
    fs = D.feat_sizes(S)
    box = [T(rng.normal(0, 0.3, (2, 36, fs[l], fs[l]))).requires_grad_(True) for l in range(3, 8)]
    cls = [T(rng.normal(0, 1, (2, 9 * D.NUM_CLASSES, fs[l], fs[l]))) for l in range(3, 8)]
    _, _, ref = D.pre_nms(cls, box, S)
    live = IO.decode(box, S)
    assert not ref.requires_grad and live.requires_grad
    assert torch.equal(ref, live.detach())


def test_teeth_every_seeded_fault_changes_the_answer():
    """tests/kernels_boxloss/boxloss_teeth (host only): the kernel checker's fp64 reference with a seeded fault
    — real centres for the far corner, a clamped gt height, a tie sent to the pred, the first tie only, no
    epsilon, the max taken over gts — must differ from the unfaulted reference on some case of its table."""
    kern = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels_boxloss")
    path = os.path.join(kern, "boxloss_teeth")
    if not os.path.isfile(path):
        if not shutil.which("g++") and not shutil.which("c++"):
            pytest.fail("tests/kernels_boxloss/boxloss_teeth is missing and there is no C++ compiler to build it")
        r = subprocess.run(["make", "-C", kern, "boxloss_teeth"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert r.returncode == 0, (r.stderr[-2000:], lines)
    assert lines[-1] == {"done": 6, "missed": 0}, lines[-1]
    seen = {d["fault"]: d["seen"] for d in lines[:-1]}
    assert seen == {k: True for k in ("real_centres", "clamp_gt", "tie_to_pred", "first_tie_only", "no_epsilon",
                                      "max_over_gts")}, seen
