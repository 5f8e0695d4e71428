"""A plain numpy fp32 restatement of the reference's training summaries (attacker.py:238-305,
attack_detection.py:252-278), written the way tf.image.draw_bounding_boxes works: box by box, in
order, four lines per box ([TF-recall], parity unpinned — TensorFlow's source is not at hand; the rules
are the ones include/phx.h states for phx_vis_sample).  It shares nothing with the kernel's per-pixel
test.
"""
import numpy as np

F = np.float32
COLOR_A = np.array([0., 1., 0.], F)  # tf.constant([[0., 1., 0.]])
COLOR_B = np.array([0., 0., 1.], F)  # tf.constant([[0., 0., 1.]])


def extents(box, H, W):
    """(min_row, min_col, max_row, max_col) of one pixel box: convert_format divides by h / w in fp32,
    the op multiplies by (height - 1) / (width - 1) in fp32 and truncates toward zero."""
    ymin, xmin, ymax, xmax = (F(v) for v in box)
    h, w = F(H), F(W)
    return (int(np.trunc(F(F(ymin / h) * F(H - 1)))), int(np.trunc(F(F(xmin / w) * F(W - 1)))),
            int(np.trunc(F(F(ymax / h) * F(H - 1)))), int(np.trunc(F(F(xmax / w) * F(W - 1)))))


def draw_one(img, box, color):
    """One box on one [H,W,3] image, in place."""
    H, W = img.shape[:2]
    min_row, min_col, max_row, max_col = extents(box, H, W)
    if min_row > max_row or min_col > max_col:
        return  # inverted
    if min_row >= H or max_row < 0 or min_col >= W or max_col < 0:
        return  # wholly outside
    r0, r1 = max(min_row, 0), min(max_row, H - 1)
    c0, c1 = max(min_col, 0), min(max_col, W - 1)
    if min_row >= 0:  # top
        for j in range(c0, c1 + 1):
            img[min_row, j] = color
    if max_row < H:   # bottom
        for j in range(c0, c1 + 1):
            img[max_row, j] = color
    if min_col >= 0:  # left
        for i in range(r0, r1 + 1):
            img[i, min_col] = color
    if max_col < W:   # right
        for i in range(r0, r1 + 1):
            img[i, max_col] = color


def draw_bounding_boxes(images, boxes, count, color):
    """images [B,H,W,3]; boxes [B,n,4] pixel boxes with count [B] valid rows: the ragged lists, padded by
    to_tensor() with zero boxes to the batch's longest.  Returns a new array."""
    out = np.array(images, F, copy=True)
    count = np.clip(np.asarray(count, np.int64), 0, boxes.shape[1])
    width = int(count.max()) if len(count) else 0
    for b in range(out.shape[0]):
        for k in range(width):
            box = boxes[b, k] if k < count[b] else np.zeros(4, F)
            draw_one(out[b], box, color)
    return out


def sample(images, boxes_a=None, count_a=None, boxes_b=None, count_b=None, *, mean, std):
    """The "Sample" image: set A drawn in [0,1,0], set B over it in [0,0,1], then
    clip(x * stddev_rgb + mean_rgb, 0, 255) cast to uint8 (truncating), every step rounding in fp32."""
    x = np.array(images, F, copy=True)
    if boxes_a is not None:
        x = draw_bounding_boxes(x, np.asarray(boxes_a, F), count_a, COLOR_A)
    if boxes_b is not None:
        x = draw_bounding_boxes(x, np.asarray(boxes_b, F), count_b, COLOR_B)
    y = (x * np.asarray(std, F)).astype(F) + np.asarray(mean, F)
    return np.clip(y.astype(F), F(0), F(255)).astype(np.uint8)


def curve_counts(scores, count, thresholds):
    """#scores >= t over the first count[b] entries of every row of [B,N], per threshold (int32 [T])."""
    scores = np.asarray(scores, F)
    count = np.arange(scores.shape[1])[None, :] < np.asarray(count).reshape(-1, 1)
    return np.array([int(((scores >= F(t)) & count).sum()) for t in np.asarray(thresholds, F)], np.int32)


def asr(num, den):
    """calc_asr from the two counts: 1 - 4n / (4d + epsilon) in float32 (tf.size of [n,4] boxes)."""
    return (F(1.0) - (F(4.0) * np.asarray(num).astype(F)) / (F(4.0) * np.asarray(den).astype(F) + F(1e-7))).astype(F)
