"""GPU tests of the validator path: rtod_score_detections (csrc/match.hip) against the fixtures recorded from the reference's
test.py and against tests/validate_ref.py, and DarknetValidator end to end on a small network.  Every comparison is an integer or
a bit-for-bit one: there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from realtimeobjectdetection_amd import cfgs, synth, validate as V
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text

pytestmark = pytest.mark.gpu

KEYS = ("people_num", "tp", "fp", "fn")


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "validate.npz"))
    out = []
    for idx, name in enumerate(g["case_names"].tolist()):
        k = "c%02d_" % idx
        out.append(dict(name=name, **{f: g[k + f] for f in ("rows", "targets", "thr", "matrix", "scores")}))
    return {"cases": out, "permitted": tuple(g["permitted"].tolist()), "min_box": int(g["min_box_size"])}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def score(images, thr, permitted=(0,), min_box=24, num_class=80, cap=None, totals=None, declared=None):
    """One rtod_score_detections call on ``images`` = [(rows [D,8], targets [T,5+C])]; everything back on the host."""
    rows = [np.asarray(r, np.float32).reshape(-1, 8) for r, _ in images]
    per = [len(r) for r in rows]
    D = sum(per)
    cap = max(D, 1) if cap is None else cap
    buf = np.zeros((cap, 8), np.float32)
    buf[:min(D, cap)] = np.concatenate(rows)[:cap]
    counts = torch.tensor([D if declared is None else declared, D] + per + [0, 0], dtype=torch.int32).cuda()
    dev_rows = torch.from_numpy(buf).cuda()
    targets = [torch.from_numpy(np.asarray(t, np.float32).reshape(-1, 5 + num_class)) for _, t in images]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scores, match, miou, _ = V.score_detections_async(dev_rows, counts, targets, num_class, permitted, min_box, thr, totals=totals, status=status)
    max_t = V.score_limits()[1]
    ws, _ = V._score_workspace(dev_rows.device, len(images), cap, max_t)
    ld = (min(max(cap, 1), V.score_limits()[0]) + 63) // 64 * 64
    M = ws.view(torch.float32)[:len(images) * max_t * ld].reshape(len(images), max_t, ld).cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(per)])
    return {"scores": scores.cpu().numpy(), "match": match.cpu().numpy(), "miou": miou.cpu().numpy(), "status": int(status.item()), "M": M, "starts": starts}


def check_image(got, b, ref, tag):
    """Image b of a call against validate_ref.score_image's dict: scores, assignment, matched IoUs, the thresholded matrix."""
    s0, n = got["starts"][b], len(ref["match"])
    assert got["scores"][b].tolist() == [ref[k] for k in KEYS], tag
    assert np.array_equal(got["match"][s0:s0 + n], ref["match"]), tag
    assert np.array_equal(bits(got["miou"][s0:s0 + n]), bits(ref["match_iou"])), tag
    P, T = ref["matrix"].shape
    if P and T:
        assert np.array_equal(bits(got["M"][b, :T, :P].T), bits(ref["matrix"])), tag


def test_every_golden_case(golden):
    for c in golden["cases"]:
        thr = float(c["thr"])
        got = score([(c["rows"], c["targets"])], thr, golden["permitted"], golden["min_box"])
        assert got["status"] == 0 and got["scores"][0].tolist() == c["scores"].tolist(), c["name"]
        ref = R.score_image(c["rows"], c["targets"], golden["permitted"], golden["min_box"], thr)
        check_image(got, 0, ref, c["name"])
        if c["matrix"].size:
            P, T = c["matrix"].shape
            assert np.array_equal(bits(got["M"][0, :T, :P].T), bits(c["matrix"])), c["name"]     # the reference's own matrix


def test_batch_packing_does_not_change_an_image(golden):
    want = ["dup_both", "dup_preds_T_gt_P", "min_box_edge", "classes", "greedy_order", "no_detections", "seed_1000", "seed_1012"]
    eight = [c for n in want for c in golden["cases"] if c["name"] == n]
    assert len(eight) == 8 and all(float(c["thr"]) == 0.5 for c in eight)
    imgs = [(c["rows"], c["targets"]) for c in eight]
    refs = [R.score_image(r, t, golden["permitted"], golden["min_box"], 0.5) for r, t in imgs]
    totals = torch.zeros(4, dtype=torch.int32, device="cuda")
    packed = score(imgs, 0.5, golden["permitted"], golden["min_box"], totals=totals)
    assert packed["status"] == 0
    once = totals.cpu().tolist()
    assert once == [sum(int(c["scores"][q]) for c in eight) for q in range(4)]
    rev = score(imgs[::-1], 0.5, golden["permitted"], golden["min_box"], totals=totals)
    assert totals.cpu().tolist() == [2 * v for v in once]                                   # accumulated over two calls
    for b, (c, ref) in enumerate(zip(eight, refs)):
        single = score([imgs[b]], 0.5, golden["permitted"], golden["min_box"])
        for got, idx in ((single, 0), (packed, b), (rev, 7 - b)):
            assert got["scores"][idx].tolist() == c["scores"].tolist(), c["name"]
            check_image(got, idx, ref, c["name"])


def _grid_image(P, T, seed, grid=4.0, classes=80):
    """T targets and P predictions scattered around them, every coordinate on a ``grid``: equal IoUs and exact duplicates occur."""
    rng = np.random.default_rng(seed)
    q = lambda v: np.round(v / grid) * grid
    t = np.zeros((T, 5 + classes), np.float32)
    t[:, 0:2] = q(rng.uniform(60, 540, (T, 2)))
    t[:, 2:4] = q(rng.uniform(20, 120, (T, 2)))                      # some at or under min_box_size
    t[:, 4] = 1
    t[np.arange(T), 5 + rng.choice([0, 0, 0, 0, 0, 3], T)] = 1
    src = t[rng.integers(0, T, P)]
    j = q(rng.normal(0, 8, (P, 4)))
    rows = np.zeros((P, 8), np.float32)
    rows[:, 1] = src[:, 0] - src[:, 2] / 2 + j[:, 0]
    rows[:, 2] = src[:, 1] - src[:, 3] / 2 + j[:, 1]
    rows[:, 3] = src[:, 0] + src[:, 2] / 2 + j[:, 2]
    rows[:, 4] = src[:, 1] + src[:, 3] / 2 + j[:, 3]
    rows[:, 5:7] = rng.uniform(0.5, 1, (P, 2))
    rows[:, 7] = rng.choice([0, 0, 0, 0, 0, 0, 0, 5], P)
    rows[P // 2:P // 2 + P // 10] = rows[:P // 10]                   # exact duplicates
    return rows, t


def test_one_large_image_with_ties():
    """300 x 40: several waves of predictions, many rounds of the matching loop, ties from the coordinate grid."""
    rows, t = _grid_image(300, 40, seed=7)
    ref = R.score_image(rows, t, (0,), 24, 0.5)
    vals = ref["matrix"][ref["matrix"] > 0]
    assert ref["tp"] >= 10 and len(np.unique(vals)) < len(vals) and len(ref["pred_kept"]) > 192          # ties are present
    got = score([(rows, t)], 0.5)
    assert got["status"] == 0
    check_image(got, 0, ref, "300x40")


def test_an_image_exactly_at_the_limits_beside_a_small_one():
    max_p, max_t = V.score_limits()
    rows, t = _grid_image(max_p, max_t, seed=9, grid=2.0)
    rows[:, 7] = 0
    t[:, 2:4] = np.maximum(t[:, 2:4], 26); t[:, 5:] = 0; t[:, 5] = 1     # every row and target is kept: P_f, T_f at the limits
    small = _grid_image(37, 5, seed=10)
    refs = [R.score_image(rows, t, (0,), 24, 0.3), R.score_image(*small, (0,), 24, 0.3)]
    assert refs[0]["people_num"] == max_t and refs[0]["tp"] + refs[0]["fp"] == max_p
    got = score([(rows, t), small], 0.3)
    assert got["status"] == 0
    for b, ref in enumerate(refs):
        check_image(got, b, ref, "limits %d" % b)


def test_status_words_are_defined_outcomes():
    max_p, max_t = V.score_limits()
    rows, t = _grid_image(12, 4, seed=3)
    # 1: more detections than the row buffer holds: every score -1, totals untouched
    totals = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    got = score([(rows, t)], 0.5, cap=8, declared=12, totals=totals)
    assert got["status"] == 1 and (got["scores"] == -1).all() and totals.cpu().tolist() == [7, 7, 7, 7]
    # 2: one image over a limit: that image alone is refused
    over_t = np.zeros((max_t + 1, 85), np.float32); over_t[:, 0:2] = 100; over_t[:, 2:4] = 50; over_t[:, 4:6] = 1
    over_p = np.zeros((max_p + 1, 8), np.float32); over_p[:, 1:5] = (10, 10, 60, 60)
    ref = R.score_image(rows, t, (0,), 24, 0.5)
    totals = torch.zeros(4, dtype=torch.int32, device="cuda")
    got = score([(rows, t), (rows, over_t), (over_p, t), (rows, t)], 0.5, totals=totals)
    assert got["status"] == 2
    assert got["scores"][1].tolist() == [-1] * 4 and got["scores"][2].tolist() == [-1] * 4
    check_image(got, 0, ref, "beside an over-limit image")
    check_image(got, 3, ref, "after an over-limit image")
    assert totals.cpu().tolist() == [2 * ref[k] for k in KEYS]
    assert set(got["match"][got["starts"][2]:got["starts"][3]].tolist()) == {-1}               # filtered, not matched


def test_compare_boxes_equals_the_reference_tp(golden):
    v = V.DarknetValidator()
    n = 0
    for c in golden["cases"]:
        pf = v.pred_filter(torch.from_numpy(c["rows"]).cuda() if len(c["rows"]) else 0, golden["permitted"])
        tf = v.target_filter(torch.from_numpy(c["targets"]).cuda(), golden["permitted"], min_box_size=golden["min_box"])
        if isinstance(pf, int) or tf is None:
            continue
        assert v.compare_boxes(pf, tf, float(c["thr"])) == int(c["scores"][1]), c["name"]
        n += 1
    assert n >= 25
    w = V.DarknetValidator(validation_thresh=0.75)                      # ... and through get_img_scores, the reference's call path
    c = next(c for c in golden["cases"] if c["name"] == "seed_1017")
    w.validation_thresh = float(c["thr"])
    w.get_img_scores("x", w.pred_filter(torch.from_numpy(c["rows"]).cuda(), [0]), w.target_filter(torch.from_numpy(c["targets"]).cuda(), [0], 24), img_scores=True)
    assert [w.image_scores["x"][k] for k in KEYS] == c["scores"].tolist() == [w.total_scores[k] for k in KEYS]


def test_validate_json_from_stored_detections(golden):
    cs = [c for c in golden["cases"] if float(c["thr"]) == 0.5]
    v = V.DarknetValidator()
    v.validate_json({c["name"]: c["rows"].tolist() for c in cs}, {c["name"]: torch.from_numpy(c["targets"]) for c in cs}, img_scores=True, batch_size=5)
    for c in cs:
        assert [v.image_scores[c["name"]][k] for k in KEYS] == c["scores"].tolist(), c["name"]
    tot = [sum(int(c["scores"][q]) for c in cs) for q in range(4)]
    assert [v.total_scores[k] for k in KEYS] == tot
    tp, fp, fn = (torch.tensor(tot[q]).float() for q in (1, 2, 3))
    assert v.precision.dtype == torch.float32 and torch.equal(v.precision, tp / (tp + fp)) and torch.equal(v.recall, tp / (tp + fn))
    assert torch.equal(v.f_score, 2 / ((1 / v.recall) + (1 / v.precision)))


# ------------------------------------------------------------------------------------------ end to end on a small network
@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    """cfgs.mini_cfg at 64x64 with synthetic weights in eval mode, four frames, the confidence lowered until the network yields
    detections, and ground truth made from those detections: jittered, every third dropped, distractors added."""
    from realtimeobjectdetection_amd.darknet import Darknet
    from realtimeobjectdetection_amd.util import write_results
    res, B = 64, 4
    text = cfgs.mini_cfg(res, res)
    ir = build_ir(parse_cfg_text(text), res)
    d = tmp_path_factory.mktemp("validate_mini")
    m = Darknet(cfgs.write_cfg(str(d / "m.cfg"), text), True).eval()
    m.net_info["height"] = res
    m.precision = "fp32"
    m.load_weight_stream(synth.synth_weights(ir))
    x = torch.from_numpy(synth.synth_frames(B, res, seed=5)).cuda()
    with torch.no_grad():
        y = m(x)
    det, conf = 0, None
    for conf in (0.5, 0.25, 0.1, 0.03, 0.01, 0.003, 0.001):
        det = write_results(y, 80, conf, 0.5)
        if not isinstance(det, int) and det.size(0) >= 16 and len(set(det[:, 0].tolist())) == B:
            break
    assert not isinstance(det, int) and det.size(0) >= 16, "the synthetic network yields no detections"
    det = det.cpu().numpy()
    cls, n = np.unique(det[:, 7], return_counts=True)
    permitted = tuple(int(c) for c in cls[np.argsort(-n, kind="stable")][:max(1, (len(cls) + 1) // 2)])
    rng = np.random.default_rng(21)
    targets = []
    for b in range(B):
        rows = det[det[:, 0] == b]
        t = []
        for i, r in enumerate(rows):
            if i % 3 == 2:
                continue
            box = r[1:5] + rng.normal(0, 1.5, 4)
            one = np.zeros(85, np.float32)
            one[:5] = ((box[0] + box[2]) / 2, (box[1] + box[3]) / 2, box[2] - box[0], box[3] - box[1], 1)
            one[5 + int(r[7])] = 1
            t.append(one)
        for k in range(3):                                           # distractors: far away, too small, another class
            one = np.zeros(85, np.float32)
            one[:5] = [(500 + 40 * k, 500, 60, 60, 1), (20, 20, 8, 8, 1), (32, 32, 40, 40, 1)][k]
            one[5 + (permitted[0] if k < 2 else (permitted[0] + 1) % 80)] = 1
            t.append(one)
        targets.append(torch.from_numpy(np.stack(t)))
    return {"model": m, "x": x, "targets": targets, "conf": conf, "permitted": permitted, "names": ["f%d" % b for b in range(B)], "y": y}


def _fresh(mini, **kw):
    a = dict(confidence=mini["conf"], nms_thresh=0.5, resolution=64, permitted_classes=mini["permitted"], min_box_size=4)
    a.update(kw)
    return V.DarknetValidator(**a)


def _batches(mini, bs):
    return [(mini["names"][i:i + bs], mini["x"][i:i + bs], mini["targets"][i:i + bs]) for i in range(0, 4, bs)]


def _expected(mini, conf, nms):
    """validate_ref on write_results' rows of the same forward."""
    from realtimeobjectdetection_amd.util import write_results
    det = write_results(mini["y"], 80, conf, nms)
    det = np.zeros((0, 8), np.float32) if isinstance(det, int) else det.cpu().numpy()
    return [R.score_image(det[det[:, 0] == b], mini["targets"][b].numpy(), mini["permitted"], 4, 0.5) for b in range(4)]


def test_validate_model_end_to_end(mini, capsys):
    per = _expected(mini, mini["conf"], 0.5)
    want = R.totals(per)
    assert want["tp"] > 0 and want["fp"] > 0 and want["fn"] > 0, want          # the ground truth exercises every count
    for bs in (1, 2, 4):
        v = _fresh(mini)
        v.validate_model(mini["model"], _batches(mini, bs), CUDA=True)
        assert v.total_scores == want, bs
        assert v.image_scores == {}
        tp, fp, fn = (torch.tensor(want[k]).float() for k in ("tp", "fp", "fn"))
        assert v.precision.dtype == torch.float32 and torch.equal(v.precision, tp / (tp + fp)) and torch.equal(v.recall, tp / (tp + fn))
        assert torch.equal(v.f_score, 2 / ((1 / v.recall) + (1 / v.precision)))
    v = _fresh(mini)
    v.validate_model(mini["model"], _batches(mini, 2), CUDA=True, img_scores=True)
    assert v.total_scores == want and set(v.image_scores) == set(mini["names"])
    for b, name in enumerate(mini["names"]):
        assert v.image_scores[name] == {k: per[b][k] for k in KEYS}             # the reference's keys
    assert "Precision" in capsys.readouterr().out


def test_sweep_equals_one_fresh_validator_per_setting(mini):
    nmss, confs = [0.3, 0.5, 0.7], [mini["conf"], min(0.9, mini["conf"] * 4)]
    for kw, settings in ((dict(nms_thresholds=nmss), [(mini["conf"], n) for n in nmss]), (dict(confidences=confs), [(c, 0.5) for c in confs])):
        got = _fresh(mini).sweep(mini["model"], _batches(mini, 4), **kw)
        assert len(got) == len(settings)
        for g, (conf, nms) in zip(got, settings):
            v = _fresh(mini, confidence=conf, nms_thresh=nms)
            v.validate_model(mini["model"], _batches(mini, 2), CUDA=True)
            assert {k: g[k] for k in KEYS} == v.total_scores == R.totals(_expected(mini, conf, nms)), (conf, nms)
            assert (g["confidence"], g["nms_thresh"]) == (conf, nms)
            for k, t in (("precision", v.precision), ("recall", v.recall), ("f_score", v.f_score)):
                assert g[k].dtype == torch.float32 and torch.equal(torch.nan_to_num(g[k], nan=-1.0), torch.nan_to_num(t, nan=-1.0))
