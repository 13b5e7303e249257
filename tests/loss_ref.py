"""The training loss's targets and value restated for the tests (numpy float64 and integers), independent of librtod and of the
product's host mirrors.  Pinned to the reference by tests/golden/yolo_loss.npz (tests/test_loss_host.py); the GPU tests use it
where the fixture cannot reach (general grids, rectangular heads, any number of anchors and classes, the out-of-grid rule).

Rules (per image, per head (GH, GW, stride, anchors); a box row is (cx, cy, w, h, conf, one-hot[C]) in float32):
  * a box counts if its class-0 slot (column 5) is exactly 1 and neither w nor h is below ``min_box`` (float32 compare);
  * its anchor is the FIRST one with the largest IoU between (w, h) and a square whose side is the anchor's WIDTH (doubles);
  * cell: x = cx / stride in double, gx = trunc(x), fx = x - gx; y likewise.  A cell outside [0, GW) x [0, GH) (negative
    coordinates and NaN included) drops the box for that head and sets status bit 0;
  * row n = (gy * GW + gx) * A + anchor behind the rows of the earlier heads;
  * the row's target is the box row with columns 0..3 replaced by (float32(fy), float32(fx), tw, th): y first;
    tw = float32(log(float64(q))) with q = float32(w) / float32(anchor_w) + float32(1e-16) in float32, th with the anchor's height;
  * a later box replaces an earlier one on the same row.
Loss: 5 * sum_obj of columns 0-1, 5 * sum_obj of columns 2-3, sum_obj of column 4, 0.5 * sum_noobj of column 4, sum_obj of
columns 5.., each a sum of (pred - target)^2 in float64; the total adds them in that order.
"""
import math

import numpy as np

F = np.float32
NAMES = ("xy", "wh", "obj", "noobj", "cls")
WEIGHTS = (5.0, 5.0, 1.0, 0.5, 1.0)


def head_rows(heads):
    return [gh * gw * len(anchors) for gh, gw, _, anchors in heads]


def fit_anchor(w, h, anchors):
    w, h = float(w), float(h)
    best, best_iou = 0, None
    for i, (aw, _) in enumerate(anchors):
        side = float(aw)
        inter = min(w, side) * min(h, side)
        iou = inter / (w * h + side * side - inter)
        if best_iou is None or iou > best_iou:
            best, best_iou = i, iou
    return best


def log_ratio(v, anchor):
    """(q, float32(log(float64(q)))) for q = float32 quotient + float32(1e-16)."""
    q = F(F(v) / F(anchor)) + F(1e-16)
    q = F(q)
    return q, (F(math.log(float(q))) if q > 0 else F(-np.inf) if q == 0 else F(np.nan))


def assign(boxes, heads, min_box=24):
    """One image: ``(owner {row: box index}, info {row: (head, anchor)}, status)``."""
    boxes = np.asarray(boxes, F).reshape(len(boxes), -1) if len(boxes) else np.zeros((0, 6), F)
    owner, info, status = {}, {}, 0
    for i, b in enumerate(boxes):
        if b[5] != F(1) or b[2] < F(min_box) or b[3] < F(min_box):
            continue
        off = 0
        for hi, (gh, gw, stride, anchors) in enumerate(heads):
            a = fit_anchor(b[2], b[3], anchors)
            x, y = float(b[0]) / stride, float(b[1]) / stride
            if 0.0 <= x < gw and 0.0 <= y < gh:
                n = off + (int(y) * gw + int(x)) * len(anchors) + a
                owner[n] = i
                info[n] = (hi, a)
            else:
                status |= 1
            off += gh * gw * len(anchors)
    return owner, info, status


def target_row(box, head, a):
    gh, gw, stride, anchors = head
    box = np.asarray(box, F)
    x, y = float(box[0]) / stride, float(box[1]) / stride
    row = box.copy()
    row[0], row[1] = F(y - int(y)), F(x - int(x))
    row[2] = log_ratio(box[2], anchors[a][0])[1]
    row[3] = log_ratio(box[3], anchors[a][1])[1]
    return row


def sparse_targets(boxes, heads, min_box=24):
    """One image: ``(rows int64 [K] ascending, target float32 [K, attrs], status)``."""
    owner, info, status = assign(boxes, heads, min_box)
    rows = np.asarray(sorted(owner), np.int64)
    boxes = np.asarray(boxes, F).reshape(len(boxes), -1) if len(boxes) else np.zeros((0, 6), F)
    tgt = np.zeros((len(rows), boxes.shape[1]), F)
    for k, n in enumerate(rows):
        hi, a = info[int(n)]
        tgt[k] = target_row(boxes[owner[int(n)]], heads[hi], a)
    return rows, tgt, status


def dense_targets(batch_boxes, heads, attrs, min_box=24):
    """``(target float32 [B,N,attrs], mask bool [B,N], n_obj [B], status)`` — what target_creator returns."""
    N = sum(head_rows(heads))
    target = np.zeros((len(batch_boxes), N, attrs), F)
    mask = np.zeros((len(batch_boxes), N), bool)
    status = 0
    for b, boxes in enumerate(batch_boxes):
        rows, tgt, st = sparse_targets(boxes, heads, min_box)
        status |= st
        if len(rows):
            target[b, rows] = tgt
            mask[b, rows] = True
    return target, mask, mask.sum(1), status


def components(pred, target, mask):
    """float64 [6] = total, xy, wh, obj, noobj, cls, and the number of summed terms of the five components."""
    p, t, m = np.asarray(pred, np.float64), np.asarray(target, np.float64), np.asarray(mask, bool)
    d = p - t
    sq = d * d
    obj, no = sq[m], sq[~m]
    raw = [obj[:, 0:2].sum(), obj[:, 2:4].sum(), obj[:, 4].sum(), no[:, 4].sum(), obj[:, 5:].sum()]
    comp = [w * float(v) for w, v in zip(WEIGHTS, raw)]
    total = comp[0]
    for v in comp[1:]:
        total = total + v
    K, C = int(m.sum()), p.shape[-1] - 5
    terms = [2 * K, 2 * K, K, int(m.size) - K, K * C]
    return np.asarray([total] + comp, np.float64), terms


def sum_bound(value, terms):
    """|device - host| allowed for a double-accumulated sum of ``terms`` non-negative summands: 2 n 2^-53 relative."""
    return 2.0 * terms * 2.0 ** -53 * abs(float(value))


def ulp_distance(a, b):
    """Distance in float32 ulps (units in the last place counted on the integer line of the encodings)."""
    def key(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
