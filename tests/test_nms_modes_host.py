"""nms_configs beyond the default, host side (no GPU): the test-side restatement of NonMaxSuppressionV5 and
per_class_nms (tests/nms_modes_oracle.py) against an independent definition and the existing oracle, the decision
margins of the random cases, VictimConfig.override's plumbing against a stub context, and the teeth of the kernel
harness's reference (tests/kernels_nms_seg/nms_seg_teeth)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import nms_modes_oracle as NO
from oracle import postprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels_nms_seg")
f32 = np.float32


def random_case(seed, n, equal=False, dup=False):
    rng = np.random.default_rng(seed)
    y, x = rng.uniform(0, 400, n), rng.uniform(0, 400, n)
    h, w = rng.uniform(8, 128, n), rng.uniform(8, 128, n)
    boxes = np.stack([y, x, y + h, x + w], 1).astype(f32)
    scores = rng.uniform(0.002, 0.998, n).astype(f32)
    if equal:
        scores[:] = 0.75
    if dup:
        boxes[1::4], boxes[2::4], boxes[3::4] = boxes[0::4][:len(boxes[1::4])], boxes[0::4][:len(boxes[2::4])], \
            boxes[0::4][:len(boxes[3::4])]
    return boxes, scores


# (name, seed, n, generator flags, iou_threshold, score_threshold, max_out); the seeds are chosen so that the
# restatement alone keeps the margins test_margins asserts
HARD_CASES = [
    ("n1", 11, 1, {}, 0.5, 0.001, 100),
    ("n63", 12, 63, {}, 0.5, 0.001, 100),
    ("n64", 13, 64, {}, 0.5, 0.001, 100),
    ("n65", 14, 65, {}, 0.5, 0.001, 100),
    ("n257", 115, 257, {}, 0.5, 0.001, 100),
    ("n257_mo7", 16, 257, {}, 0.5, 0.001, 7),
    ("n257_mo1", 17, 257, {}, 0.5, 0.001, 1),
    ("n257_thresh_half", 218, 257, {}, 0.5, 0.5, 100),
    ("n257_thresh_neg_inf", 219, 257, {}, 0.5, float("-inf"), 100),
    ("n600_iou03", 320, 600, {}, 0.3, 0.001, 100),
    ("n600_iou07", 721, 600, {}, 0.7, 0.001, 100),
]
# the planted exact-equality cases: the only exceptions to the margins (score ties decided by the index; IoU 1
# against threshold 1; IoU exactly at the threshold, and one ulp above it)
PLANTED = [
    ("equal_scores", 30, 257, {"equal": True}, 0.5, 0.001, 100),
    ("duplicates_iou1", 31, 256, {"dup": True}, 1.0, 0.001, 100),
    ("duplicates", 32, 256, {"dup": True}, 0.5, 0.001, 100),
    ("iou0", 33, 257, {}, 0.0, 0.001, 100),
]
HALF = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [100, 100, 110, 110]], f32)             # IoU(0, 1) = 50 / 100
HALF_ULP = np.array([[0, 0, 4095, 4093], [0, 0, 4094, 2047], [5000, 5000, 5010, 5010]], f32)  # 8380418 / 16760835


@pytest.mark.parametrize("case", HARD_CASES + PLANTED, ids=lambda c: c[0])
def test_restatement_equals_brute_force_hard_nms(case):
    _, seed, n, flags, iou, thr, mo = case
    boxes, scores = random_case(seed, n, **flags)
    idx, sc = NO.nms_v5(boxes, scores, mo, iou, thr, 0.0)
    bidx, bsc = NO.hard_nms_brute(boxes, scores, mo, iou, thr)
    np.testing.assert_array_equal(idx, bidx)
    np.testing.assert_array_equal(sc, bsc)
    assert len(idx) <= mo and (n < 2 or len(idx) >= 1)


def test_iou_exactly_at_the_threshold_survives_and_one_ulp_above_goes():
    sc = np.array([0.9, 0.8, 0.7], f32)
    assert pp._iou(HALF[0], HALF[1]) == f32(0.5)
    assert pp._iou(HALF_ULP[0], HALF_ULP[1]) == np.nextafter(f32(0.5), f32(1))
    for fn in (lambda b: NO.nms_v5(b, sc, 100, 0.5, 0.001, 0.0), lambda b: NO.hard_nms_brute(b, sc, 100, 0.5, 0.001)):
        assert list(fn(HALF)[0]) == [0, 1, 2]        # sim > iou_threshold is strict
        assert list(fn(HALF_ULP)[0]) == [0, 2]


@pytest.mark.parametrize("case", HARD_CASES + PLANTED, ids=lambda c: c[0])
def test_restatement_equals_the_existing_soft_oracle(case):
    _, seed, n, flags, _, thr, mo = case
    if thr == float("-inf"):
        thr = 0.001  # the existing oracle's candidates are scores > a finite threshold
    boxes, scores = random_case(seed, n, **flags)
    idx, sc = NO.nms_v5(boxes, scores, mo, 1.0, thr, 0.25)
    oidx, osc = pp.soft_nms(boxes, scores, mo, thr, 0.25)
    np.testing.assert_array_equal(idx, oidx)
    np.testing.assert_array_equal(sc, osc)


def test_effective_thresholds_follow_postprocess_nms():
    assert NO.effective("hard", None, 0.0, None) == (f32(0.5), f32("-inf"), f32(0))
    assert NO.effective("", 0.3, 0.25, 0.7) == (f32(0.3), f32(0.25), f32(0))
    assert NO.effective(None, None, 0.5, None) == (f32(0.5), f32(0.5), f32(0))
    assert NO.effective("gaussian", 0.3, 0.0, None) == (f32(1), f32(0.001), f32(0.25))
    assert NO.effective("gaussian", None, 0.4, 0.3) == (f32(1), f32(0.4), f32(0.15))
    with pytest.raises(ValueError):
        NO.effective("linear", None, 0, None)


def test_margins_of_the_random_cases():
    """Every IoU comparison of a hard case lies at least 1e-5 from the threshold, and every decayed-score comparison
    of the soft runs at least 8 error bounds from what it is compared with, so an fp32 evaluation that rounds
    differently (another expf) decides the same.  The planted cases are the exceptions, by name."""
    for name, seed, n, flags, iou, thr, mo in HARD_CASES:
        boxes, scores = random_case(seed, n, **flags)
        tr = NO.Trace()
        NO.nms_v5(boxes, scores, mo, iou, thr, 0.0, trace=tr)
        print(name, "iou gap", tr.iou_gap, "pops", tr.pops, "drops", tr.drops)
        assert tr.iou_gap >= 1e-5, (name, tr.iou_gap)
        tr = NO.Trace()
        NO.nms_v5(boxes, scores, mo, 1.0, 0.001 if thr == float("-inf") else thr, 0.25, trace=tr)
        print(name, "score margin", tr.score_margin, "requeues", tr.requeues)
        assert tr.score_margin >= 8, (name, tr.score_margin)
    gaps = {}
    for name, seed, n, flags, iou, thr, mo in PLANTED:
        boxes, scores = random_case(seed, n, **flags)
        tr = NO.Trace()
        NO.nms_v5(boxes, scores, mo, iou, thr, 0.0, trace=tr)
        gaps[name] = (tr.iou_gap, tr.tie_pops)
    assert gaps["equal_scores"][1] > 0                                   # ties: the index decides
    assert gaps["duplicates_iou1"][0] == 0 and gaps["duplicates"][0] > 0  # IoU 1 at threshold 1: kept
    assert gaps["iou0"][0] == 0                                           # IoU 0 at threshold 0: kept


def test_per_class_merge_order_valid_len_and_no_clip():
    # classes 2 and 5; class 5's best outranks class 2's second; one box reaches outside the image
    boxes = np.array([[-20, -30, 40, 50], [100, 100, 150, 150], [300, 300, 360, 380], [100, 100, 150, 150],
                      [200, 10, 260, 60]], f32)
    scores = np.array([0.9, 0.6, 0.8, 0.6, 0.0005], f32)
    classes = np.array([2, 2, 5, 5, 7])
    ob, os_, oc, n = NO.per_class_nms(boxes, scores, classes, 90, 100, 0.5, 0.001, 0.0, image_scale=2.0)
    assert n == 4                                              # the 0.0005 candidate is below the threshold
    np.testing.assert_array_equal(os_[:4], f32([0.9, 0.8, 0.6, 0.6]))
    np.testing.assert_array_equal(oc[:5], f32([3, 6, 3, 6, 0]))   # the 0.6 tie: class 2 (lower position) first
    np.testing.assert_array_equal(ob[0], f32([-40, -60, 80, 100]))  # x image_scale, not clipped
    assert not ob[4:].any() and not os_[4:].any()
    # max_output_size 3: per class at most 3, merged to 3, valid_len capped
    ob3, os3, oc3, n3 = NO.per_class_nms(boxes, scores, classes, 90, 3, 0.5, 0.001, 0.0)
    assert n3 == 3 and list(oc3[:4]) == [3, 6, 3, 0] and not ob3[3:].any()
    # max_output_size 1: each class keeps its best only
    _, os1, oc1, n1 = NO.per_class_nms(boxes, scores, classes, 90, 1, 0.5, 0.001, 0.0)
    assert n1 == 1 and os1[0] == f32(0.9) and oc1[0] == 3
    # a class outside [0, num_classes) belongs to no NMS
    _, _, oc9, n9 = NO.per_class_nms(boxes, scores, np.array([2, 2, 95, 95, 7]), 90, 100, 0.5, 0.001, 0.0)
    assert n9 == 2 and list(oc9[:3]) == [3, 3, 0]
    # nothing above the threshold
    assert NO.per_class_nms(boxes, scores * 0, classes, 90, 100, 0.5, 0.001, 0.0)[3] == 0
    # gaussian: the same boxes in two classes decay alike; the tie goes to the lower class again
    b2 = np.concatenate([boxes[:2], boxes[:2]])
    b2[1] = b2[3] = [-10, -20, 45, 55]
    _, osg, ocg, ng = NO.per_class_nms(b2, f32([0.9, 0.8, 0.9, 0.8]), np.array([1, 1, 4, 4]), 90, 100, 1.0, 0.001, 0.25)
    assert ng == 4 and list(ocg[:4]) == [2, 5, 2, 5] and osg[2] == osg[3] < f32(0.8)


class StubCtx:
    def __init__(self):
        self.calls = []

    def set_score_thresh(self, t):
        self.calls.append(("score_thresh", t))

    def set_nms_config(self, **kw):
        self.calls.append(("nms", kw))


def _config(**kw):
    from mladversarialobjectdetection_amd.attacker import NmsConfig, VictimConfig
    return VictimConfig("efficientdet-d0", 128, [0] * 3, [1] * 3, NmsConfig(), **kw)


def test_override_forwards_the_nms_settings():
    ctx = StubCtx()
    c = _config(ctx=ctx, honour_nms_configs=True)
    c.override({"nms_configs": {"method": "hard", "iou_thresh": .5, "score_thresh": .25, "sigma": 0.3,
                                "max_output_size": 10}})
    assert ctx.calls == [("nms", {"method": "hard"}), ("nms", {"iou_thresh": .5}), ("score_thresh", .25),
                         ("nms", {"sigma": 0.3}), ("nms", {"max_output_size": 10})]
    assert (c.nms_configs.method, c.nms_configs.iou_thresh, c.nms_configs.sigma, c.nms_configs.max_output_size) == \
        ("hard", .5, 0.3, 10)
    for method, want in (("", "hard"), (None, "hard"), ("gaussian", "gaussian")):
        ctx.calls.clear()
        c.override({"nms_configs": {"method": method}})
        assert ctx.calls == [("nms", {"method": want})] and c.nms_configs.method == method
    ctx.calls.clear()
    c.override({"nms_configs": {"iou_thresh": None, "sigma": None}})   # "or 0.5" on both
    assert ctx.calls == [("nms", {"iou_thresh": 0.0}), ("nms", {"sigma": 0.5})]


def test_override_keeps_refusing_what_is_not_built():
    ctx = StubCtx()
    c = _config(ctx=ctx, honour_nms_configs=True)
    for bad, word in (({"pyfunc": True}, "pyfunc"), ({"max_nms_inputs": 5000}, "max_nms_inputs"),
                      ({"max_output_size": 101}, "max_output_size is fixed at 100"), ({"method": "linear"}, "invalid nms method"),
                      ({"max_output_size": 0}, "max_output_size"), ({"foo": 1}, "unsupported nms_configs key")):
        with pytest.raises(ValueError, match=word):
            c.override({"nms_configs": bad})
    c.override({"nms_configs": {"pyfunc": False, "max_nms_inputs": 0}})
    assert ctx.calls == []
    with pytest.raises(ValueError, match="library context"):
        _config(honour_nms_configs=True).override({"nms_configs": {"method": "hard"}})
    # without honour_nms_configs the settings are refused as before, and iou_thresh is ignored
    old = _config(ctx=ctx)
    old.override({"nms_configs": {"iou_thresh": .5}})
    assert ctx.calls == []
    for bad in ({"method": "hard"}, {"sigma": 0.3}, {"max_output_size": 50}):
        with pytest.raises(ValueError):
            old.override({"nms_configs": bad})


def test_context_validates_and_reports_the_nms_config():
    """phx_set_nms_config / phx_set_post_mode on a context without weights: host-side validation, the thresholds in
    force whichever setter comes first, and phx_model_info's report."""
    from mladversarialobjectdetection_amd import _lib
    ctx = _lib.Context("efficientdet-d0", image_size=128, max_batch=1, score_thresh=0.0)
    info = ctx.model_info()
    assert info["nms_method"] == "gaussian" and info["nms_score_thresh"] == pytest.approx(0.001)
    assert info["nms_iou_thresh"] == 1 and info["nms_sigma"] == 0.5 and info["nms_max_output_size"] == 100
    assert info["post_mode"] == "global" and ctx.get_post_mode() == "global"
    assert ctx.get_nms_config() == {"method": "gaussian", "iou_thresh": 0.0, "sigma": 0.5, "max_output_size": 100}
    ctx.set_nms_config(method="hard")
    info = ctx.model_info()
    assert info["nms_method"] == "hard" and info["nms_score_thresh"] is None and info["nms_iou_thresh"] == 0.5
    ctx.set_score_thresh(0.25)
    a = ctx.model_info()
    other = _lib.Context("efficientdet-d0", image_size=128, max_batch=1, score_thresh=0.0)
    other.set_score_thresh(0.25)
    other.set_nms_config(method="hard")
    assert a == other.model_info() and a["nms_score_thresh"] == pytest.approx(0.25)
    ctx.set_nms_config(method="gaussian", sigma=0.3, max_output_size=10, iou_thresh=0.7)
    info = ctx.model_info()
    assert (info["nms_iou_thresh"], info["nms_max_output_size"]) == (1, 10) and info["nms_sigma"] == pytest.approx(0.3)
    ctx.set_score_thresh(0.0)
    assert ctx.model_info()["nms_score_thresh"] == pytest.approx(0.001)
    for bad in ({"max_output_size": 101}, {"max_output_size": 0}, {"iou_thresh": 1.5}, {"iou_thresh": -0.1},
                {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": float("nan")}):
        with pytest.raises(_lib.PhxError):
            ctx.set_nms_config(**bad)
    with pytest.raises(_lib.PhxError, match="100"):
        ctx.set_nms_config(max_output_size=101)
    assert ctx.get_nms_config()["max_output_size"] == 10   # a refused call changes nothing
    ctx.set_post_mode("per_class")
    assert ctx.model_info()["post_mode"] == "per_class" and ctx.get_post_mode() == "per_class"
    with pytest.raises(ValueError):
        ctx.set_post_mode("combined")
    assert ctx.lib.phx_set_post_mode(ctx.h, 7) != 0


def test_teeth_every_seeded_fault_trips():
    """nms_seg_teeth: the kernel harness's reference with a seeded fault must change the answer on some case of the
    table — '>=' for '>' at the IoU threshold, ties by the higher index, visits oldest first, a clip in per-class,
    merge ties by class descending, valid_len not capped."""
    path = os.path.join(KERN, "nms_seg_teeth")
    if not os.path.isfile(path):
        if not shutil.which("g++") and not shutil.which("c++"):
            pytest.fail("tests/kernels_nms_seg/nms_seg_teeth is missing and there is no C++ compiler to build it")
        r = subprocess.run(["make", "-C", KERN, "nms_seg_teeth"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert lines[-1] == {"done": 6, "all_tripped": True, "clean_trips": 0}, lines[-1]
    faults = {d["fault"]: d["tripped"] for d in lines[:-1]}
    assert set(faults) == {"iou_ge", "tie_hi", "visit_oldest", "pc_clip", "merge_class_desc", "valid_uncapped"}
    assert all(v > 0 for v in faults.values()), faults
