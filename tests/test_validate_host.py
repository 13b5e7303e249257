"""CPU tests of the validator path: the numpy restatement (tests/validate_ref.py) against fixtures recorded from the reference's
test.py (tests/golden/validate.npz, written by tests/golden/make_golden_validate.py), CocoTargets against the reference's COCO
class, the host-side refusals of rtod_score_detections, and the host class's conventions.  No device call is made."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from realtimeobjectdetection_amd import _ffi
from realtimeobjectdetection_amd.validate import CocoTargets, DarknetValidator, score_limits


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "validate.npz"))


def cases(g):
    for idx, name in enumerate(g["case_names"].tolist()):
        k = "c%02d_" % idx
        yield name, {f: g[k + f] for f in ("rows", "targets", "thr", "tf", "pf", "matrix", "scores")}


def test_fixture_covers_the_cases_the_arithmetic_can_get_wrong(golden):
    names = golden["case_names"].tolist()
    assert len(names) >= 30 and {float(c["thr"]) for _, c in cases(golden)} == {0.5, 0.3, 0.75}
    by = dict(cases(golden))
    assert by["iou_eq_050"]["matrix"].max() == 0 and by["iou_eq_075"]["matrix"].max() == 0          # IoU == threshold: no match
    assert by["iou_f32_030"]["matrix"][0, 0] == np.float32(0.3)                                      # float32(0.3) > 0.3 in double
    assert len(by["min_box_edge"]["tf"]) == 2 and len(by["classes"]["tf"]) == 1 and len(by["classes"]["pf"]) == 2
    assert any(len(c["pf"]) > len(c["tf"]) > 0 for _, c in cases(golden)) and any(len(c["tf"]) > len(c["pf"]) > 0 for _, c in cases(golden))
    assert len(by["preds_filtered_away"]["pf"]) == 0 and len(by["targets_filtered_away"]["tf"]) == 0
    dup = by["dup_both"]["matrix"]
    assert dup.shape == (3, 2) and (dup == dup[0, 0]).all() and dup[0, 0] == 1.0                    # every entry ties


def test_validate_ref_equals_the_reference_on_every_case(golden):
    permitted = tuple(golden["permitted"].tolist())
    mb = int(golden["min_box_size"])
    for name, c in cases(golden):
        s = R.score_image(c["rows"], c["targets"], permitted, mb, float(c["thr"]))
        assert np.array_equal(s["target_boxes"].view(np.uint32), c["tf"].view(np.uint32)), name
        assert np.array_equal(c["rows"][s["pred_kept"]].view(np.uint32), c["pf"].view(np.uint32)), name
        if len(c["pf"]) and len(c["tf"]):
            assert s["matrix"].shape == c["matrix"].shape and np.array_equal(s["matrix"].view(np.uint32), c["matrix"].view(np.uint32)), name
        assert [s["people_num"], s["tp"], s["fp"], s["fn"]] == c["scores"].tolist(), name
        assert int((s["match"] >= 0).sum()) == s["tp"] and len(set(s["match"][s["match"] >= 0].tolist())) == s["tp"], name


def test_coco_targets_equal_the_reference_bit_for_bit(golden, tmp_path):
    from PIL import Image
    ann = json.loads(bytes(golden["coco_json"]).decode())
    for im in ann["images"]:
        Image.new("RGB", (im["width"], im["height"]), (90, 120, 150)).save(str(tmp_path / im["file_name"]))
    json.dump(ann, open(str(tmp_path / "ann.json"), "w"))
    ds = CocoTargets(str(tmp_path / "ann.json"), str(tmp_path), int(golden["coco_resolution"]), batch_size=2)
    want_names = golden["coco_names"].tolist()
    assert len(ds) == len(want_names) == 3
    for i, n in enumerate(want_names):
        name, t = ds.targets(i)
        assert name == n and t.dtype == torch.float32
        assert np.array_equal(t.numpy().view(np.uint32), golden["coco_t%d" % i].view(np.uint32)), n
    seen = []
    for names, frames, targets in ds:                       # three sizes: no two images share a batch
        assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) == len(names) == len(targets)
        size = {(im["height"], im["width"]) for im in ann["images"] if im["file_name"] in names}
        assert size == {(frames.size(1), frames.size(2))}
        for n, t in zip(names, targets):
            assert np.array_equal(t.numpy().view(np.uint32), golden["coco_t%d" % want_names.index(n)].view(np.uint32))
        seen += names
    assert seen == want_names
    assert set(ds.targets_by_name()) == set(want_names)


def _call(**over):
    """rtod_score_detections with fake (never dereferenced) device addresses: every refusal is decided on the host."""
    lib = _ffi.lib()
    need = C.c_size_t()
    assert lib.rtod_score_detections_workspace(2, 64, 256, C.byref(need)) == 0
    a = dict(det=4096, counts=4096, cap=64, batch=2, tgt=4096, toff=4096, num_class=80, mask=(C.c_uint32 * 3)(1, 0, 0), min_box=24.0, thr=0.5,
             max_tgt=256, corners=0, scores=4096, totals=None, match=None, miou=None, status=4096, ws=4096, ws_bytes=need.value)
    a.update(over)
    p = lambda v: None if v is None else C.c_void_p(v)
    return lib.rtod_score_detections(p(a["det"]), p(a["counts"]), a["cap"], a["batch"], p(a["tgt"]), p(a["toff"]), a["num_class"], a["mask"], a["min_box"],
                                     a["thr"], a["max_tgt"], a["corners"], p(a["scores"]), p(a["totals"]), p(a["match"]), p(a["miou"]), p(a["status"]),
                                     p(a["ws"]), a["ws_bytes"], None)


def test_limits_and_workspace_are_host_arithmetic():
    lib = _ffi.lib()
    max_p, max_t = score_limits()
    assert max_p >= 1024 and max_t >= 256
    assert lib.rtod_score_detections_limits(None, None) == -1 and "null" in _ffi.last_error()
    need = C.c_size_t()
    assert lib.rtod_score_detections_workspace(8, 16384, max_t, C.byref(need)) == 0
    assert need.value == 8 * max_t * min(16384, max_p) * 4                 # the thresholded matrices, [batch][targets][predictions]
    assert lib.rtod_score_detections_workspace(1, 0, 1, C.byref(need)) == 0 and need.value == 64 * 4
    for bad in ((0, 64, 256), (1, -1, 256), (1, 64, 0), (1, 64, max_t + 1)):
        assert lib.rtod_score_detections_workspace(*bad, C.byref(need)) == -1 and "score_detections_workspace" in _ffi.last_error()
    assert lib.rtod_score_detections_workspace(1, 64, 256, None) == -1


@pytest.mark.parametrize("over,word", [
    (dict(det=None), "null"), (dict(counts=None), "null"), (dict(tgt=None), "null"), (dict(toff=None), "null"), (dict(mask=None), "null"),
    (dict(scores=None), "null"), (dict(status=None), "null"), (dict(ws=None), "null"),
    (dict(batch=0), "batch"), (dict(cap=-1), "cap"), (dict(num_class=0), "classes"), (dict(num_class=4097), "classes"),
    (dict(max_tgt=0), "max_targets_per_image"), (dict(max_tgt=257), "max_targets_per_image"),
    (dict(thr=float("nan")), "not a number"), (dict(ws_bytes=1023), "too small"), (dict(ws=4100), "aligned"), (dict(det=4100), "aligned"),
])
def test_score_detections_refuses_bad_arguments_on_the_host(over, word):
    assert _call(**over) == -1
    assert word in _ffi.last_error() and "score_detections" in _ffi.last_error()


def test_validator_has_no_cpu_path():
    v = DarknetValidator()
    rows, tg = torch.zeros(2, 8), torch.zeros(2, 85)
    for call in (lambda: v.compare_boxes(rows, tg, 0.5), lambda: v.score_batch(rows, torch.zeros(4, dtype=torch.int32), [tg]),
                 lambda: v.validate_model(None, [], CUDA=False)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_constructor_and_filters_keep_the_reference_conventions(golden):
    v = DarknetValidator()
    assert (v.confidence, v.num_classes, v.nms_thresh, v.validation_thresh, v.resolution) == (0.6, 80, 0.5, 0.5, 416)
    assert (v.permitted_classes, v.min_box_size) == ((0,), 24)
    assert v.image_scores == {} and v.total_scores == {"people_num": 0, "tp": 0, "fn": 0, "fp": 0}
    for bad in (dict(resolution=400), dict(resolution=416.0), dict(confidence=1.5), dict(nms_thresh=-0.1)):
        with pytest.raises(AssertionError):
            DarknetValidator(**bad)
    permitted = golden["permitted"].tolist()
    for name, c in cases(golden):
        tf = v.target_filter(torch.from_numpy(c["targets"]), permitted, min_box_size=int(golden["min_box_size"]))
        if len(c["tf"]) == 0:
            assert tf is None, name
        else:
            assert np.array_equal(tf.numpy().view(np.uint32), c["tf"].view(np.uint32)), name
        pf = v.pred_filter(torch.from_numpy(c["rows"]) if len(c["rows"]) else 0, permitted)
        if len(c["pf"]) == 0:
            assert type(pf) == int and pf == 0, name
        else:
            assert np.array_equal(pf.numpy().view(np.uint32), c["pf"].view(np.uint32)), name
    # get_img_scores' branches that need no matching, and the bookkeeping methods
    v.get_img_scores("none", 0, None, img_scores=True)
    assert v.image_scores == {} and v.total_scores["people_num"] == 0
    v.get_img_scores("miss", 0, torch.zeros(3, 85), img_scores=True)
    v.get_img_scores("fp", torch.zeros(2, 8), None, img_scores=True)
    assert v.image_scores == {"miss": {"people_num": 3, "tp": 0, "fp": 0, "fn": 3}, "fp": {"people_num": 0, "tp": 0, "fp": 2, "fn": 0}}
    assert v.total_scores == {"people_num": 3, "tp": 0, "fn": 3, "fp": 2}


def test_cli_usage_names_validate():
    from realtimeobjectdetection_amd import __main__ as M
    with pytest.raises(SystemExit) as e:
        M.main(["frobnicate"])
    assert "validate" in str(e.value) and "detect" in str(e.value)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with pytest.raises(SystemExit) as e:                       # the shipped params.json names no validation set
        M.main(["validate", os.path.join(root, "params.json")])
    assert "valid_annot_dir" in str(e.value) and "valid_img_dir" in str(e.value)
