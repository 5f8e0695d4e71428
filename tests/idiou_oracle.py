"""InverseDIOULoss (regression_loss.py:16-142) restated for the tests (a helper, not a test), fp64.

The module, taken as written:

* `InverseDIOULoss.__call__(boxes_pred, boxes_true)` (:27-68): per image, `reduce_max` over the predicted
  boxes (axis 0 of the [P, G] map, :54) of `1. - diou_loss(gt, pred)` (:84), `reduce_sum` over the gts
  (:55); 0 when the image has no predicted box (:58-59); `+ keras.backend.epsilon()` = 1e-7 per image
  (:59); the batch value is the sum over images (:61).
* `diou_loss(b1 = gt, b1_area, b1_height, b1_width, b2 = pred)` (:101-142): the gt's height, width and
  area come from `__call__` unclamped (:45-47); the pred's width and height are clamped at 0 (:115-116);
  `iou = divide_no_nan(intersect_area, union_area)` (:128); the "centres" are
  `(ymin + height, xmin + width)` (:130-131: the far corner, as written); `enclose_diag` is the sum of
  the squared clamped enclosing height and width (:134-140); `diou = iou - divide_no_nan(center_dist,
  enclose_diag)` (:141); the function returns `1. - diou` (:142) and the caller `1. -` that (:84).

Gradient rules [TF-recall] (TensorFlow's registered gradients, restated from memory of math_grad.py):

* `reduce_max` (_MaxGrad): the gradient is split equally among the elements equal to the maximum.
* `tf.maximum(x, y)` / `tf.minimum(x, y)` (_MaximumMinimumGrad): x takes the gradient where x >= y
  (x <= y), y only where it wins strictly.  In `diou_loss` the gt (or the constant 0.) is always x, so a
  pred coordinate gets gradient only on a strict win and `maximum(0., v)` passes only v > 0.
* `divide_no_nan` (_DivNoNanGrad): both gradients are 0 where the denominator is 0.

The predicted set and the wiring are the library's (the reference never wired the module in): inside the
tape of PatchAttacker.call, `loss += w * InverseDIOULoss()(boxes_pred, boxes)` with boxes_pred the second
pass's anchors of argmax class 0 that pass filter_valid_boxes(thresh=False) (attacker.py:118-141) and
boxes the placement boxes.  The masks are constants; the gradient reaches the network through
decode_box_outputs (tf2/anchors.py:30-58) only.  `oracle.detector.pre_nms` detaches the box tensor, so
`decode` below decodes again without the detach.
"""
import numpy as np
import torch

from oracle import detector as D
from oracle import eot
from oracle import postprocess as pp
from oracle import step as ST

EPS = 1e-7  # keras.backend.epsilon()


def tf_max(x, y):
    """tf.maximum(x, y) with TF's gradient: x where x >= y."""
    x, y = torch.broadcast_tensors(torch.as_tensor(x, dtype=y.dtype) if not torch.is_tensor(x) else x, y)
    return torch.where(x >= y, x, y)


def tf_min(x, y):
    x, y = torch.broadcast_tensors(torch.as_tensor(x, dtype=y.dtype) if not torch.is_tensor(x) else x, y)
    return torch.where(x <= y, x, y)


def div_no_nan(x, y):
    zero = y == 0
    safe = torch.where(zero, torch.ones_like(y), y)
    return torch.where(zero, torch.zeros_like(x * y), x / safe)


def idiou_pairs(gt, pred):
    """[G, P] map of 1. - diou_loss(b1 = gt[g], b2 = pred[p]) (regression_loss.py:84, :101-142)."""
    gt = gt.reshape(-1, 1, 4)
    pred = pred.reshape(1, -1, 4)
    g_ymin, g_xmin, g_ymax, g_xmax = gt.unbind(-1)
    p_ymin, p_xmin, p_ymax, p_xmax = pred.unbind(-1)
    g_h = g_ymax - g_ymin  # :45-47, not clamped
    g_w = g_xmax - g_xmin
    g_area = g_h * g_w
    zero = torch.zeros((), dtype=pred.dtype)
    p_w = tf_max(zero, p_xmax - p_xmin)
    p_h = tf_max(zero, p_ymax - p_ymin)
    p_area = p_w * p_h
    i_ymin = tf_max(g_ymin, p_ymin)
    i_xmin = tf_max(g_xmin, p_xmin)
    i_ymax = tf_min(g_ymax, p_ymax)
    i_xmax = tf_min(g_xmax, p_xmax)
    i_w = tf_max(zero, i_xmax - i_xmin)
    i_h = tf_max(zero, i_ymax - i_ymin)
    i_area = i_w * i_h
    union = g_area + p_area - i_area
    iou = div_no_nan(i_area, union)
    dist = ((g_ymin + g_h) - (p_ymin + p_h)) ** 2 + ((g_xmin + g_w) - (p_xmin + p_w)) ** 2  # :130-132
    e_ymin = tf_min(g_ymin, p_ymin)
    e_xmin = tf_min(g_xmin, p_xmin)
    e_ymax = tf_max(g_ymax, p_ymax)
    e_xmax = tf_max(g_xmax, p_xmax)
    e_w = tf_max(zero, e_xmax - e_xmin)
    e_h = tf_max(zero, e_ymax - e_ymin)
    diag = e_h ** 2 + e_w ** 2
    diou = iou - div_no_nan(dist, diag)
    return 1.0 - (1.0 - diou)


def idiou_image(gt, pred):
    """The image's value (regression_loss.py:49-59): sum_g max_p + epsilon; 0 + epsilon without a pred."""
    gt = torch.as_tensor(gt).reshape(-1, 4)
    pred = pred.reshape(-1, 4)
    if pred.shape[0] == 0 or gt.shape[0] == 0:
        return pred.sum() * 0.0 + EPS  # (a reduce_sum over no gts is 0)
    return D.TieMax.apply(idiou_pairs(gt.to(pred.dtype), pred)).sum() + EPS


def idiou_batch(gts, preds):
    """InverseDIOULoss()(boxes_pred, boxes_true): the sum over images (:61, :66)."""
    return sum(idiou_image(g, p) for g, p in zip(gts, preds))


def idiou_loops(gt, pred):
    """The image's value by a loop-for-loop numpy transcription: for every pred, for every gt (:87-99,
    :71-84), diou_loss term by term; reduce_max over preds, reduce_sum over gts, + epsilon."""
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    pred = np.asarray(pred, np.float64).reshape(-1, 4)

    def dnn(x, y):
        return 0.0 if y == 0 else x / y

    if len(pred) == 0:
        return 0.0 + EPS
    rows = []
    for box in pred:
        row = []
        for ind in range(len(gt)):
            b1 = gt[ind]
            b1_height, b1_width = b1[2] - b1[0], b1[3] - b1[1]
            b1_area = b1_height * b1_width
            b2_width = max(0.0, box[3] - box[1])
            b2_height = max(0.0, box[2] - box[0])
            b2_area = b2_width * b2_height
            intersect_width = max(0.0, min(b1[3], box[3]) - max(b1[1], box[1]))
            intersect_height = max(0.0, min(b1[2], box[2]) - max(b1[0], box[0]))
            intersect_area = intersect_width * intersect_height
            iou = dnn(intersect_area, b1_area + b2_area - intersect_area)
            c1 = (b1[0] + b1_height, b1[1] + b1_width)
            c2 = (box[0] + b2_height, box[1] + b2_width)
            center_dist = (c1[0] - c2[0]) ** 2.0 + (c1[1] - c2[1]) ** 2.0
            enclose_width = max(0.0, max(b1[3], box[3]) - min(b1[1], box[1]))
            enclose_height = max(0.0, max(b1[2], box[2]) - min(b1[0], box[0]))
            enclose_diag = enclose_height ** 2.0 + enclose_width ** 2.0
            diou = iou - dnn(center_dist, enclose_diag)
            row.append(1.0 - (1.0 - diou))
        rows.append(row)
    m = np.asarray(rows, np.float64).reshape(len(pred), len(gt))
    return float(m.max(axis=0).sum()) + EPS


def decode(box_outs, image_size, anchor_scale=4.0):
    """decode_box_outputs (tf2/anchors.py:30-58) of the levels' box outputs, [B, A, 4], differentiable
    (oracle.detector.pre_nms's own decode is detached)."""
    B = box_outs[0].shape[0]
    box = torch.cat([b.permute(0, 2, 3, 1).reshape(B, -1, 4) for b in box_outs], 1)
    an = torch.as_tensor(D.anchors(image_size, anchor_scale), dtype=box.dtype)
    yca = (an[:, 0] + an[:, 2]) / 2
    xca = (an[:, 1] + an[:, 3]) / 2
    ha = an[:, 2] - an[:, 0]
    wa = an[:, 3] - an[:, 1]
    ty, tx, th, tw = box.unbind(-1)
    w = torch.exp(tw) * wa
    h = torch.exp(th) * ha
    yc = ty * ha + yca
    xc = tx * wa + xca
    return torch.stack([yc - h / 2.0, xc - w / 2.0, yc + h / 2.0, xc + w / 2.0], -1)


def attack_step(weights, images, patch, scale, boxes, seed=0, step=0, gimg0=0, model="efficientdet-d0",
                image_size=None, add_tv=True, dtype=torch.float64, training=True, bn_frozen=False):
    """oracle.step.attack_step with injected placement boxes and the box term kept apart: returns
    dict(loss0, box (the unweighted batch value), grad0, grad_box (NPARAM each: [patch | scale]; None when
    not training), per_image, pairs (per image the [G, P] map over the kept anchors, fp64 numpy),
    kept (per image the kept anchors' indices)).  The step's loss at weight w is loss0 + w * box and its
    gradient grad0 + w * grad_box."""
    image_size = image_size or D.MODELS[model]["image_size"]
    det = D.Detector(weights, model, image_size, dtype=dtype, training=training,
                     drop=dict(seed=seed, step=step, gimg0=gimg0, **{"pass": 1}), bn_frozen=bn_frozen)
    images_t = torch.as_tensor(np.asarray(images, dtype=np.float64), dtype=dtype)
    B = images_t.shape[0]
    place_boxes = [np.asarray(bx, np.float32).reshape(-1, 4) for bx in boxes]
    patch_t = torch.as_tensor(np.asarray(patch, dtype=np.float64), dtype=dtype).requires_grad_(training)
    scale_t = torch.tensor(float(np.float32(scale)), dtype=dtype, requires_grad=training)
    patched = torch.stack([eot.patch_image(images_t[b], patch_t, place_boxes[b], np.float32(scale), seed, step,
                                           gimg0 + b) for b in range(B)])
    cls, box = det(patched)
    scores, classes, dboxes = D.pre_nms(cls, box, image_size, det.cfg["anchor_scale"])
    live = decode(box, image_size, det.cfg["anchor_scale"])
    m, per_image, pairs, kept = [], [], [], []
    for b in range(B):
        keep = torch.as_tensor((classes[b].numpy() == 0)
                               & pp.valid_mask(dboxes[b].numpy().astype(np.float32), image_size, image_size))
        r = ST._ragged_max(scores[b], keep)
        m.append(torch.where(r >= 0, r, torch.zeros_like(r)))
        pred = live[b][keep]
        gt = torch.as_tensor(place_boxes[b].astype(np.float64), dtype=dtype)
        per_image.append(idiou_image(gt, pred))
        kept.append(np.nonzero(keep.numpy())[0])
        with torch.no_grad():
            pairs.append(idiou_pairs(gt, pred).numpy() if len(gt) and pred.shape[0] else np.zeros((len(gt), 0)))
    m = torch.stack(m)
    tv = (patch_t[1:, :, :] - patch_t[:-1, :, :]).abs().sum() + (patch_t[:, 1:, :] - patch_t[:, :-1, :]).abs().sum()
    loss0 = (m ** 2 + (m - scale_t) ** 2).sum()
    if add_tv:
        loss0 = loss0 + 1e-5 * tv
    boxv = sum(per_image)
    grad0 = grad_box = None
    if training:
        def flat(loss):
            gp, gs = torch.autograd.grad(loss, [patch_t, scale_t], retain_graph=True, allow_unused=True)
            gp = torch.zeros_like(patch_t) if gp is None else gp
            gs = torch.zeros_like(scale_t) if gs is None else gs
            return np.concatenate([gp.detach().numpy().reshape(-1), [gs.item()]])
        grad0 = flat(loss0)
        grad_box = flat(boxv) if boxv.requires_grad else np.zeros_like(grad0)
    return dict(loss0=loss0.item(), box=float(boxv.detach()), grad0=grad0, grad_box=grad_box,
                per_image=np.array([float(v.detach()) for v in per_image]), pairs=pairs, kept=kept)
