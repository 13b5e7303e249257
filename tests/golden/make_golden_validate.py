#!/usr/bin/env python
"""Fixtures that pin the validator to the reference (same harness as make_golden_refcheck.py):

    python tests/golden/make_golden_validate.py <reference checkout>

writes tests/golden/validate.npz.  The reference's test.py is loaded by file location (``import test`` would find the standard
library's package), with cv2 stubbed.  As committed, DarknetValidator.compare_boxes raises TypeError (its two helpers are
@staticmethods declared with a ``self`` parameter), so the validator is subclassed and only compare_boxes is overridden: it calls
the reference's own two static functions with a placeholder first argument.  Recorded per seeded case: the outputs of
target_filter and pred_filter, the thresholded IoU matrix, TP, and the four numbers the reference's get_img_scores leaves in
total_scores; and the targets of the reference's COCO class (only_ground_truth mode) for a three-image annotation file written
here.  Data only: nothing from the reference is copied."""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
C = 80
MIN_BOX = 24
PERMITTED = [0]


def tgt(cx, cy, w, h, cls=0):
    r = np.zeros(5 + C, F)
    r[:5] = (cx, cy, w, h, 1.0)
    r[5 + cls] = 1.0
    return r


def tgt_xyxy(x1, y1, x2, y2, cls=0):
    return tgt((x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1, cls)


def det(x1, y1, x2, y2, cls=0, obj=0.9, score=0.8):
    return np.asarray([0, x1, y1, x2, y2, obj, score, cls], F)


def fixed_cases():
    """(name, rows [D,8], targets [T,85], threshold)"""
    out = []
    # exact duplicate boxes on both sides: every entry of the matrix ties
    out.append(("dup_both", [det(10, 10, 69, 89)] * 3, [tgt_xyxy(10, 10, 69, 89)] * 2, 0.5))
    out.append(("dup_preds_T_gt_P", [det(10, 10, 69, 89)] * 2, [tgt_xyxy(10, 10, 69, 89), tgt_xyxy(12, 10, 71, 89), tgt_xyxy(200, 200, 259, 289), tgt_xyxy(10, 10, 69, 89)], 0.5))
    # IoU exactly at the threshold is no match (strict >): 900 / 1800, 900 / 1200; float32(900 / 3000) > 0.3 IS one (0.3 is no float32)
    out.append(("iou_eq_050", [det(0, 0, 29, 29)], [tgt_xyxy(0, 0, 29, 59)], 0.5))
    out.append(("iou_eq_075", [det(0, 0, 29, 29)], [tgt_xyxy(0, 0, 29, 39)], 0.75))
    out.append(("iou_f32_030", [det(0, 0, 29, 29)], [tgt_xyxy(0, 0, 29, 99)], 0.3))
    out.append(("iou_just_above_050", [det(0, 0, 29, 29), det(0, 0, 29, 58)], [tgt_xyxy(0, 0, 29, 59)], 0.5))
    # targets at exactly min_box_size are dropped (strict >), one pixel more is kept
    out.append(("min_box_edge", [det(100, 100, 123, 160), det(200, 100, 224, 160), det(300, 100, 360, 124)],
                [tgt(112, 130, 24, 60), tgt(212.5, 130, 25, 60), tgt(330, 112, 60, 24), tgt(330, 112.5, 60, 25)], 0.5))
    # classes that are not permitted, on both sides
    out.append(("classes", [det(10, 10, 69, 89, cls=1), det(10, 10, 69, 89, cls=0), det(100, 100, 169, 189, cls=79), det(100, 100, 169, 189)],
                [tgt_xyxy(10, 10, 69, 89, cls=2), tgt_xyxy(10, 10, 69, 89), tgt_xyxy(100, 100, 169, 189, cls=1)], 0.5))
    # either side empty after filtering, both empty, no detections at all
    out.append(("preds_filtered_away", [det(10, 10, 69, 89, cls=3)] * 2, [tgt_xyxy(10, 10, 69, 89)], 0.5))
    out.append(("targets_filtered_away", [det(10, 10, 69, 89)] * 2, [tgt(40, 50, 20, 20), tgt_xyxy(10, 10, 69, 89, cls=5)], 0.5))
    out.append(("both_filtered_away", [det(10, 10, 69, 89, cls=3)], [tgt(40, 50, 20, 20)], 0.5))
    out.append(("no_detections", [], [tgt_xyxy(10, 10, 69, 89), tgt_xyxy(100, 100, 169, 189)], 0.5))
    # the greedy order matters: p0 overlaps both targets best, p1 only the first
    out.append(("greedy_order", [det(0, 0, 59, 59), det(0, 0, 59, 69)], [tgt_xyxy(0, 0, 59, 64), tgt_xyxy(0, 0, 59, 57)], 0.5))
    return out


def seeded_cases(n=27):
    out = []
    for k in range(n):
        rng = np.random.default_rng(1000 + k)
        thr = (0.5, 0.3, 0.75)[k % 3]
        T = int(rng.integers(1, 9)); P = int(rng.integers(1, 12))
        grid = 8.0 if k % 3 == 0 else 1.0                          # a third of the cases: boxes on a coarse grid, duplicates likely
        ts, ps = [], []
        for _ in range(T):
            w, h = rng.uniform(16, 180, 2); cx, cy = rng.uniform(60, 350, 2)
            q = lambda v: float(np.round(v / grid) * grid)
            ts.append(tgt(q(cx), q(cy), q(w), q(h), cls=int(rng.choice([0, 0, 0, 0, 1, 7]))))
        for _ in range(P):
            if rng.random() < 0.75:
                t = ts[int(rng.integers(0, T))]
                j = rng.normal(0, 6.0 if grid == 1.0 else 10.0, 4)
                x1, y1, x2, y2 = t[0] - t[2] / 2 + j[0], t[1] - t[3] / 2 + j[1], t[0] + t[2] / 2 + j[2], t[1] + t[3] / 2 + j[3]
            else:
                x1, y1 = rng.uniform(0, 300, 2); x2, y2 = x1 + rng.uniform(20, 150), y1 + rng.uniform(20, 150)
            q = lambda v: float(np.round(v / grid) * grid)
            ps.append(det(q(x1), q(y1), q(x2), q(y2), cls=int(rng.choice([0, 0, 0, 0, 0, 2])), obj=float(rng.uniform(0.6, 1)), score=float(rng.uniform(0.3, 1))))
        if grid > 1.0 and P > 2:
            ps[-1] = ps[0].copy()                                  # an exact duplicate prediction
        out.append(("seed_%d" % (1000 + k), ps, ts, thr))
    return out


COCO_ANN = {
    "images": [{"id": 9, "file_name": "img_9.png", "width": 640, "height": 480},
               {"id": 25, "file_name": "img_25.png", "width": 333, "height": 500},
               {"id": 42, "file_name": "img_42.png", "width": 416, "height": 416}],
    "annotations": [
        {"image_id": 9, "iscrowd": 0, "category_id": 1, "bbox": [100.5, 50.25, 200.0, 300.75]},
        {"image_id": 9, "iscrowd": 0, "category_id": 18, "bbox": [10.0, 20.0, 30.0, 24.5]},
        {"image_id": 9, "iscrowd": 1, "category_id": 1, "bbox": [300.0, 100.0, 120.0, 200.0]},
        {"image_id": 25, "iscrowd": 0, "category_id": 1, "bbox": [33.3, 44.4, 155.5, 266.6]},
        {"image_id": 25, "iscrowd": 0, "category_id": 90, "bbox": [0.0, 0.0, 333.0, 500.0]},
        {"image_id": 42, "iscrowd": 0, "category_id": 13, "bbox": [7.0, 9.0, 100.0, 40.0]},
        {"image_id": 42, "iscrowd": 0, "category_id": 1, "bbox": [200.0, 210.0, 24.0, 25.0]},
    ],
}
COCO_RES = 416


def main(ref):
    import torch
    from PIL import Image
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref)
    spec = importlib.util.spec_from_file_location("ref_test", os.path.join(ref, "test.py"))
    ref_test = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_test)
    from src.dataset import COCO

    class Validator(ref_test.DarknetValidator):
        def compare_boxes(self, pred, target, threshold):
            m = ref_test.DarknetValidator.create_iou_matrix_for_predictions_and_targets(None, [], pred, [], target, threshold)
            self.last_matrix = m.clone()
            return ref_test.DarknetValidator.evaluate_iou_matrix(None, m, pred, 0)

    out = {}
    with tempfile.TemporaryDirectory() as d:
        ann = os.path.join(d, "ann.json")
        json.dump(COCO_ANN, open(ann, "w"))
        for im in COCO_ANN["images"]:
            Image.new("RGB", (im["width"], im["height"]), (90, 120, 150)).save(os.path.join(d, im["file_name"]))
        cases = fixed_cases() + seeded_cases()
        names = []
        for idx, (name, ps, ts, thr) in enumerate(cases):
            v = Validator(ann, d, validation_thresh=thr)
            rows = np.stack(ps).astype(F) if len(ps) else np.zeros((0, 8), F)
            targets = np.stack(ts).astype(F)
            v.last_matrix = torch.zeros(0, 0)
            tf = v.target_filter(torch.from_numpy(targets), PERMITTED, min_box_size=MIN_BOX)
            pf = v.pred_filter(torch.from_numpy(rows) if len(rows) else 0, PERMITTED)
            v.get_img_scores(name, pf, tf, img_scores=True)
            s = v.image_scores.get(name, {"people_num": 0, "tp": 0, "fp": 0, "fn": 0})
            assert s == {k: v.total_scores[k] for k in s}
            k = "c%02d_" % idx
            names.append(name)
            out[k + "rows"] = rows
            out[k + "targets"] = targets
            out[k + "thr"] = np.float64(thr)
            out[k + "tf"] = tf.numpy() if tf is not None else np.zeros((0, 5 + C), F)
            out[k + "pf"] = pf.numpy() if not isinstance(pf, int) else np.zeros((0, 8), F)
            out[k + "matrix"] = v.last_matrix.numpy().astype(F)
            out[k + "scores"] = np.asarray([s["people_num"], s["tp"], s["fp"], s["fn"]], np.int64)
        out["case_names"] = np.asarray(names)
        out["min_box_size"] = np.int64(MIN_BOX)
        out["permitted"] = np.asarray(PERMITTED, np.int64)
        # the COCO class's targets, ground truth only, in the order of its img_ids
        ds = COCO(ann, d, COCO_RES, keep_img_name=True, only_ground_truth=True)
        coco_names = []
        for i in range(len(ds)):
            name, bbox = ds[i]
            coco_names.append(name)
            out["coco_t%d" % i] = bbox.numpy()
        out["coco_names"] = np.asarray(coco_names)
        out["coco_json"] = np.frombuffer(json.dumps(COCO_ANN).encode(), np.uint8)
        out["coco_resolution"] = np.int64(COCO_RES)
    path = os.path.join(HERE, "validate.npz")
    np.savez_compressed(path, **out)
    print(len(names), "cases,", os.path.getsize(path), "bytes;", {n: out["c%02d_scores" % i].tolist() for i, n in enumerate(names)})


if __name__ == "__main__":
    main(sys.argv[1])
