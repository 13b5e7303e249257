"""numpy restatement of the reference validator's arithmetic (test.py:62-151, 182-208), float32 operation by operation:
target_filter / pred_filter, the thresholded IoU matrix of create_iou_matrix_for_predictions_and_targets, the greedy matching of
evaluate_iou_matrix with torch's first-occurrence max / argmax, and get_img_scores' four numbers.  The yardstick of
tests/test_validate_host.py (against fixtures recorded from the reference) and of tests/test_validate_gpu.py (against the kernel)."""
import numpy as np

F = np.float32


def bbox_iou(a, b):
    """bbox_iou(box1, box2) of src/util.py:120-153 for two float32 boxes (x1, y1, x2, y2): +1 pixel convention, one rounding per op."""
    a = np.asarray(a, F); b = np.asarray(b, F)
    ix1, iy1 = max(a[0], b[0]), max(a[1], b[1])
    ix2, iy2 = min(a[2], b[2]), min(a[3], b[3])
    iw = max(F(F(ix2 - ix1) + F(1)), F(0))
    ih = max(F(F(iy2 - iy1) + F(1)), F(0))
    inter = F(iw * ih)
    a1 = F(F(F(a[2] - a[0]) + F(1)) * F(F(a[3] - a[1]) + F(1)))
    a2 = F(F(F(b[2] - b[0]) + F(1)) * F(F(b[3] - b[1]) + F(1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return F(inter / F(F(a1 + a2) - inter))


def target_filter(target, permitted_classes, min_box_size=0):
    """-> (indices of the kept rows, their rows with columns 0-3 turned into corners like xywh2xyxy)."""
    t = np.asarray(target, F).reshape(-1, np.shape(target)[-1] if np.ndim(target) == 2 else 5)
    mb = F(min_box_size)
    keep = [i for i in range(len(t)) if t[i, 2] > mb and t[i, 3] > mb and int(np.argmax(t[i, 5:])) in permitted_classes]
    out = t[keep].copy()
    if keep:
        k = t[keep]
        out[:, 0] = k[:, 0] - k[:, 2] / F(2)
        out[:, 1] = k[:, 1] - k[:, 3] / F(2)
        out[:, 2] = k[:, 0] + k[:, 2] / F(2)
        out[:, 3] = k[:, 1] + k[:, 3] / F(2)
    return np.asarray(keep, np.int64), out


def pred_filter(rows, permitted_classes):
    """-> indices of the rows whose last column equals a permitted class (``pred[i, -1] in permitted_classes``)."""
    r = np.asarray(rows, F).reshape(-1, 8)
    return np.asarray([i for i in range(len(r)) if any(r[i, -1] == F(c) for c in permitted_classes)], np.int64)


def iou_matrix(pred, tbox, threshold):
    """float32 [P, T]: iou where float(iou) > threshold (a double compare of the float32 value, ``iou.item() > threshold``), else 0.
    bbox_iou above, element-wise on float32 arrays (the same single rounding per operation)."""
    p = np.asarray(pred, F).reshape(-1, np.shape(pred)[-1] if np.ndim(pred) == 2 else 8)[:, None, 1:5]
    t = np.asarray(tbox, F).reshape(-1, np.shape(tbox)[-1] if np.ndim(tbox) == 2 else 4)[None, :, 0:4]
    one, zero = F(1), F(0)
    iw = np.maximum((np.minimum(p[..., 2], t[..., 2]) - np.maximum(p[..., 0], t[..., 0])) + one, zero)
    ih = np.maximum((np.minimum(p[..., 3], t[..., 3]) - np.maximum(p[..., 1], t[..., 1])) + one, zero)
    inter = iw * ih
    a1 = ((p[..., 2] - p[..., 0]) + one) * ((p[..., 3] - p[..., 1]) + one)
    a2 = ((t[..., 2] - t[..., 0]) + one) * ((t[..., 3] - t[..., 1]) + one)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / ((a1 + a2) - inter)
    assert iou.dtype == F
    return np.where(iou.astype(np.float64) > float(threshold), iou, zero).astype(F)


def greedy_match(M):
    """evaluate_iou_matrix: -> (tp, assignment[P] = matched column or -1, matched IoU[P])."""
    M = np.array(M, F)
    P = M.shape[0]
    assign = np.full(P, -1, np.int64)
    ious = np.zeros(P, F)
    tp = 0
    for _ in range(P):
        if M.size == 0 or M.max() == 0:
            break
        max_val = M.max(axis=1)
        max_ind = M.argmax(axis=1)                 # first occurrence, like torch.max(dim=1) on the CPU
        i = int(np.argmax(max_val))                # first occurrence
        j = int(max_ind[i])
        assign[i], ious[i] = j, M[i, j]
        M[i, :] = 0
        M[:, j] = 0
        tp += 1
    return tp, assign, ious


def score_image(rows, target, permitted_classes=(0,), min_box_size=24, threshold=0.5):
    """One image: detection rows [D, 8] (or None / 0 for none) and targets [T, 5+C] -> dict with the four scores, the
    per-row match (-2 filtered, -1 unmatched, else index into the unfiltered targets), the matched IoUs and the matrix."""
    rows = np.zeros((0, 8), F) if rows is None or isinstance(rows, int) else np.asarray(rows, F).reshape(-1, 8)
    target = np.asarray(target, F)
    if target.ndim != 2:
        target = target.reshape(0, 6)
    pk = pred_filter(rows, permitted_classes)
    tk, tb = target_filter(target, permitted_classes, min_box_size)
    M = iou_matrix(rows[pk], tb, threshold)
    tp, assign, ious = greedy_match(M) if len(pk) and len(tk) else (0, np.full(len(pk), -1, np.int64), np.zeros(len(pk), F))
    match = np.full(len(rows), -2, np.int64)
    miou = np.zeros(len(rows), F)
    for i, r in enumerate(pk):
        match[r] = tk[assign[i]] if assign[i] >= 0 else -1
        miou[r] = ious[i]
    return {"people_num": len(tk), "tp": tp, "fp": len(pk) - tp, "fn": len(tk) - tp, "match": match, "match_iou": miou,
            "matrix": M, "pred_kept": pk, "target_kept": tk, "target_boxes": tb}


def totals(images):
    return {k: sum(int(s[k]) for s in images) for k in ("people_num", "tp", "fp", "fn")}
