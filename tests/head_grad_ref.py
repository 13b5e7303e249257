"""The gradient of the training loss with respect to the raw head maps, restated for the tests in numpy float64: the closed form
that autograd gives through the reference's predict_transform(TRAIN=True) and darknet_loss.  Independent of librtod and of
torch; pinned to the reference's own autograd by tests/golden/yolo_loss_grad.npz (tests/test_head_grad_host.py).  Targets and
masks come from tests/loss_ref.py.

Per prediction row p (TRAIN=True decode: sigmoid on columns 0, 1, 4.., identity on 2, 3), target row t, w = (5, 5, 5, 5, 1, 1, ...):
  object row     g_c = 2 w_c (p_c - t_c)
  no-object row  g_4 = p_4 (= 2 * 0.5 * (p_4 - 0)), every other g_c = 0
  dz_c = g_c p_c (1 - p_c) on the sigmoid columns, dz_c = g_c on columns 2, 3
Raw map channel a * attrs + c at cell (gy, gx) of a head <-> prediction row (gy * GW + gx) * A + a of that head.

``scale`` is the magnitude the subtraction's operands carry, D_c = 2 w_c (|p_c| + |t_c|) s_c with s_c = p_c (1 - p_c) or 1 (w = 0.5 and
t = 0 on a no-object row): float32 rounding errors of g and dz are a few 2^-24 of it, whatever cancels in p - t.
"""
import numpy as np

import loss_ref as R

F = np.float32


def sigmoid(v):
    v = np.asarray(v, np.float64)
    return 1.0 / (1.0 + np.exp(-v))


def rows_from_raw(raw, A, attrs):
    """[B, A*attrs, GH, GW] -> [B, GH*GW*A, attrs] (predict_transform's reshuffle), any dtype."""
    B, _, GH, GW = raw.shape
    return raw.reshape(B, A, attrs, GH * GW).transpose(0, 3, 1, 2).reshape(B, GH * GW * A, attrs)


def raw_from_rows(rows, A, GH, GW):
    """The inverse: [B, GH*GW*A, attrs] -> [B, A*attrs, GH, GW]."""
    B, _, attrs = rows.shape
    return rows.reshape(B, GH * GW, A, attrs).transpose(0, 2, 3, 1).reshape(B, A * attrs, GH, GW)


def train_decode(raws, heads):
    """Raw maps (one [B, A*attrs, GH, GW] per head) -> the TRAIN=True prediction tensor [B, N, attrs] in float64."""
    out = []
    for raw, (gh, gw, _, anchors) in zip(raws, heads):
        A = len(anchors)
        p = rows_from_raw(np.asarray(raw, np.float64), A, raw.shape[1] // A).copy()
        p[..., :2] = sigmoid(p[..., :2])
        p[..., 4:] = sigmoid(p[..., 4:])
        out.append(p)
    return np.concatenate(out, axis=1)


def weights(attrs):
    w = np.ones(attrs, np.float64)
    w[:4] = 5.0
    return w


def sig_factor(pred):
    """s_c: p (1 - p) on the sigmoid columns, 1 on columns 2, 3."""
    p = np.asarray(pred, np.float64)
    s = p * (1.0 - p)
    s[..., 2:4] = 1.0
    return s


def grad_pred(pred, target, mask):
    """g [B, N, attrs] float64: the gradient of the loss with respect to the TRAIN=True prediction tensor."""
    p, t, m = np.asarray(pred, np.float64), np.asarray(target, np.float64), np.asarray(mask, bool)
    g = np.zeros_like(p)
    g[m] = 2.0 * weights(p.shape[-1]) * (p[m] - t[m])
    g[~m, 4] = p[~m, 4]
    return g


def scale(pred, target, mask, raw):
    """D [B, N, attrs]: the operand magnitude behind g (raw=False) or dz (raw=True); 0 where the gradient is structurally 0."""
    p, t, m = np.asarray(pred, np.float64), np.asarray(target, np.float64), np.asarray(mask, bool)
    d = np.zeros_like(p)
    d[m] = 2.0 * weights(p.shape[-1]) * (np.abs(p[m]) + np.abs(t[m]))
    d[~m, 4] = np.abs(p[~m, 4])
    return d * sig_factor(p) if raw else d


def grad_raw_rows(pred, target, mask):
    """dz in the row layout [B, N, attrs] float64."""
    return grad_pred(pred, target, mask) * sig_factor(pred)


def split_heads(rows, heads):
    """[B, N, attrs] -> one [B, A*attrs, GH, GW] map per head."""
    out, off = [], 0
    for gh, gw, _, anchors in heads:
        n = gh * gw * len(anchors)
        out.append(raw_from_rows(rows[:, off:off + n], len(anchors), gh, gw))
        off += n
    return out


def loss_and_grads(raws, batch_boxes, heads, min_box=24):
    """Everything from raw maps and box lists: dict with pred, target, mask, status, components (float64 [6]), g and dz (row layout)."""
    pred = train_decode(raws, heads)
    target, mask, _, status = R.dense_targets(batch_boxes, heads, pred.shape[-1], min_box)
    comp, _ = R.components(pred, target, mask)
    return {"pred": pred, "target": target, "mask": mask, "status": status, "components": comp,
            "g": grad_pred(pred, target, mask), "dz": grad_raw_rows(pred, target, mask)}


def relative_error(value, want, d):
    """(rms, max) of (value - want) / d over the elements with d != 0; (0, 0) if there is none."""
    sel = d != 0
    if not sel.any():
        return 0.0, 0.0
    e = (np.asarray(value, np.float64)[sel] - want[sel]) / d[sel]
    return float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())
