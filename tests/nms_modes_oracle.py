"""Test-side restatement of the reference's NMS settings beyond the default, in float32.

  effective        postprocess.nms (automl/efficientdet/tf2/postprocess.py:175-188): the thresholds NonMaxSuppressionV5
                   gets from nms_configs under method 'hard' / '' / None and 'gaussian'
  nms_v5           tf.raw_ops.NonMaxSuppressionV5 for any iou_threshold / score_threshold / soft_nms_sigma: TensorFlow's
                   lazy priority queue [TF-recall], as oracle/postprocess.py:47-75 restates its soft case
  hard_nms_brute   an independent O(n^2) definition of greedy hard NMS (a different algorithm: it checks nms_v5, not
                   the kernel)
  nms_global       nms(padded=True) + clip_boxes for one image, rows at and beyond the count zero (the library's
                   convention)
  per_class_nms    per_class_nms (postprocess.py:409-467) for one image: nms(padded=False) per class, concatenation in
                   class order padded with max_output_size zero rows, tf.math.top_k, boxes x image_scale, NO clip

nms_v5 can record every comparison it decides (trace), for the margin conditions of tests/test_nms_modes_host.py: the
IoU comparisons against the threshold, and for decayed scores the running error bound of an fp32 evaluation whose only
library function, expf, is within one ulp (tests/kernels/post_check.hpp's E arithmetic).
"""
from __future__ import annotations

import heapq

import numpy as np

from oracle.postprocess import _iou

f32 = np.float32
K_U = 2.0 ** -24        # one fp32 rounding, relative
K_DEN = 7.1e-46         # half the smallest subnormal
EXP_ULP = 1.0           # expf's error in ulps (post_check.hpp's floor)


def effective(method, iou_thresh, score_thresh, sigma):
    """-> (iou_threshold, score_threshold, soft_nms_sigma) as postprocess.nms passes them."""
    if method == "hard" or not method:
        return f32(iou_thresh or 0.5), f32(score_thresh or float("-inf")), f32(0.0)
    if method == "gaussian":
        return f32(1.0), f32(score_thresh or 0.001), f32((sigma or 0.5) / 2)
    raise ValueError("Inference has invalid nms method {}".format(method))


class Trace:
    """What nms_v5 decided on: iou_gap = min |sim - iou_threshold| over the visits (hard: every visit up to the
    suppressing one; soft: every visit), score_margin = the smallest distance of a decayed-score comparison (against the
    score threshold after a decaying visit, against the runner-up at a pop when either was decayed) in units of its
    error bound, and counters."""

    def __init__(self):
        self.iou_gap = np.inf
        self.score_margin = np.inf
        self.pops = self.requeues = self.drops = self.tie_pops = 0


def _mul_e(av, ae, bv, be):
    v = av * bv
    ep = abs(av) * be + abs(bv) * ae + ae * be
    return v, ep + K_U * (abs(v) + ep) + K_DEN


def nms_v5(boxes, scores, max_output_size, iou_threshold, score_threshold, soft_nms_sigma, trace: Trace | None = None,
           cand=None):
    """-> (selected indices int64, selected scores float32).  cand: the candidate indices (default: all), any order."""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    scores = np.asarray(scores, f32).reshape(-1)
    thr, iou_t, sigma = f32(score_threshold), f32(iou_threshold), f32(soft_nms_sigma)
    soft = sigma > 0
    scale = f32(-0.5) / sigma if soft else f32(0)
    idxs = range(len(scores)) if cand is None else [int(i) for i in cand]
    # max-heap on (score desc, index asc); err = the entry's running error bound (trace only)
    heap = [(-scores[i], i, 0, 0.0) for i in idxs if scores[i] > thr]
    heapq.heapify(heap)
    selected, sel_scores = [], []
    while len(selected) < max_output_size and heap:
        negs, idx, sb, err = heapq.heappop(heap)
        score = f32(-negs)
        orig = score
        if trace is not None:
            trace.pops += 1
            if heap:
                s2, e2 = float(-heap[0][0]), heap[0][3]
                if s2 == float(orig):
                    trace.tie_pops += 1
                if err > 0 or e2 > 0:
                    trace.score_margin = min(trace.score_margin, abs(float(orig) - s2) / (err + e2))
        hard_suppress = False
        sv, se = float(score), err
        decayed = False
        for j in range(len(selected) - 1, sb - 1, -1):
            sim = _iou(boxes[idx], boxes[selected[j]])
            if trace is not None:
                trace.iou_gap = min(trace.iou_gap, abs(float(sim) - float(iou_t)))
            if soft:
                if sim <= iou_t:
                    arg = f32(f32(scale * sim) * sim)
                    w = f32(np.exp(arg))
                    if arg != 0:
                        wv = float(np.exp(np.float64(arg)))
                        sv, se = _mul_e(sv, se, wv, EXP_ULP * 2 * K_U * wv + K_DEN)
                        decayed = True
                else:
                    w = f32(0.0)
                    sv, se = 0.0, 0.0
                score = f32(score * w)
            elif sim > iou_t:
                hard_suppress = True
                break
            if score <= thr:
                break
        if trace is not None and decayed and se > 0:
            trace.score_margin = min(trace.score_margin, abs(sv - float(thr)) / se)
        sb = len(selected)
        if hard_suppress:
            if trace is not None:
                trace.drops += 1
            continue
        if score == orig:
            selected.append(idx)
            sel_scores.append(score)
            continue
        if score > thr:
            if trace is not None:
                trace.requeues += 1
            heapq.heappush(heap, (-score, idx, sb, se))
    return np.asarray(selected, np.int64), np.asarray(sel_scores, f32)


def hard_nms_brute(boxes, scores, max_output_size, iou_threshold, score_threshold):
    """Greedy hard NMS by definition: candidates sorted by (score descending, index ascending); a box is kept when its
    IoU with every kept box is <= the threshold; stop at max_output_size."""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    scores = np.asarray(scores, f32).reshape(-1)
    order = sorted((i for i in range(len(scores)) if scores[i] > f32(score_threshold)), key=lambda i: (-scores[i], i))
    kept = []
    for i in order:
        if len(kept) == max_output_size:
            break
        if all(_iou(boxes[i], boxes[k]) <= f32(iou_threshold) for k in kept):
            kept.append(i)
    return np.asarray(kept, np.int64), scores[kept].astype(f32)


def nms_global(boxes, scores, image_size, max_output_size, iou_threshold, score_threshold, soft_nms_sigma, cand=None,
               rows=100):
    """-> (boxes [rows,4] clipped to [0, image_size], scores [rows], count, selected indices)."""
    idx, sc = nms_v5(boxes, scores, max_output_size, iou_threshold, score_threshold, soft_nms_sigma, cand=cand)
    ob, os_ = np.zeros((rows, 4), f32), np.zeros(rows, f32)
    n = len(idx)
    if n:
        ob[:n] = np.clip(np.asarray(boxes, f32).reshape(-1, 4)[idx], 0, f32(image_size))
        os_[:n] = sc
    return ob, os_, n, idx


def per_class_nms(boxes, scores, classes, num_classes, max_output_size, iou_threshold, score_threshold, soft_nms_sigma,
                  image_scale=None, rows=100):
    """-> (boxes [rows,4], scores [rows], classes [rows] float32, valid_len).  Rows at and beyond valid_len are zero."""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    scores = np.asarray(scores, f32).reshape(-1)
    classes = np.asarray(classes).reshape(-1)
    cb, cs, cc, total = [], [], [], 0
    for cid in range(num_classes):
        ind = np.nonzero(classes == cid)[0]
        if len(ind) == 0:
            continue
        sel, sc = nms_v5(boxes[ind], scores[ind], max_output_size, iou_threshold, score_threshold, soft_nms_sigma)
        cb.append(boxes[ind][sel])
        cs.append(sc)
        cc.append(np.full(len(sel), cid + 1, f32))
        total += len(sel)
    pad = max_output_size
    allb = np.concatenate(cb + [np.zeros((pad, 4), f32)]) if cb else np.zeros((pad, 4), f32)
    alls = np.concatenate(cs + [np.zeros(pad, f32)]) if cs else np.zeros(pad, f32)
    allc = np.concatenate(cc + [np.zeros(pad, f32)]) if cc else np.zeros(pad, f32)
    # tf.math.top_k: value descending, ties to the lower index
    order = np.lexsort((np.arange(len(alls)), -alls.astype(np.float64)))[:max_output_size]
    valid = min(max_output_size, total)
    ob, os_, oc = np.zeros((rows, 4), f32), np.zeros(rows, f32), np.zeros(rows, f32)
    k = len(order)
    ob[:k], os_[:k], oc[:k] = allb[order], alls[order], allc[order]
    if image_scale is not None:
        ob = (ob * f32(image_scale)).astype(f32)
    ob[valid:], os_[valid:], oc[valid:] = 0, 0, 0
    return ob, os_, oc, valid
