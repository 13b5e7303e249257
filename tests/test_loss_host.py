"""Host tests of the training-loss path: tests/loss_ref.py and the DarknetTrainer host mirrors against the fixture recorded from
the reference's train.py (tests/golden/yolo_loss.npz), and the argument checks of the new entry points, which are decided on the
host.  The device itself is covered by tests/test_loss_gpu.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import loss_ref as R
from loss_cases import check_targets, load_cases
from realtimeobjectdetection_amd import _ffi, cfgs
from realtimeobjectdetection_amd.cfg import parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer, make_heads, model_heads

F = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_cases(golden_dir)


def test_fixture_holds_what_the_issue_asks_for(golden):
    g, cases = golden
    assert [c["name"] for c in cases] == ["tiny_b1", "tiny_b2", "tiny_b3", "v3_b1"]
    assert [(c["B"], c["N"]) for c in cases] == [(1, 2535), (2, 2535), (3, 2535), (1, 10647)]
    tiny = cases[0]
    # the issue's observation: a box at (101, 201) on the 13-grid, alone, gives row 243 with slots (y, x) = (0.28125, 0.15625)
    rows, tgt, _ = R.sparse_targets(np.asarray([tiny["images"][0][0]]), tiny["heads"][:1])
    assert rows.tolist() == [243] and tgt[0, :2].tolist() == [0.28125, 0.15625]
    for (w, h), fit in zip(g["probe_wh"].tolist(), g["probe_fit"].tolist()):
        assert R.fit_anchor(w, h, tiny["heads"][0][3]) == fit
    boxes = tiny["images"][0]
    assert (boxes[:, 2] == F(23.9)).any() and (boxes[:, 3] == F(23.9)).any() and ((boxes[:, 2] == 24) & (boxes[:, 3] == 24)).any()
    assert (boxes[:, 5] != 1).any()
    assert any(len(im) == 0 for c in cases for im in c["images"])                       # an image without boxes
    assert any(len(im) and len(R.assign(im, c["heads"])[0]) == 0 for c in cases for im in c["images"])   # one whose boxes are all filtered
    assert all((im[:, :2] >= 0).all() and (im[:, :2] < 416).all() for c in cases for im in c["images"] if len(im))
    # collisions: fewer masked rows than (kept boxes) x (heads); a centre on a stride multiple: fractions 0
    owner, _, _ = R.assign(boxes, tiny["heads"])
    kept = int(((boxes[:, 5] == 1) & (boxes[:, 2] >= 24) & (boxes[:, 3] >= 24)).sum())
    assert len(owner) < kept * len(tiny["heads"])
    assert (tiny["target_rows"][:, :2] == 0).all(axis=1).any()
    # the anchor's height would have mattered, and an exact tie goes to the first anchor
    w, h = g["height_matters_wh"].tolist()
    differs = False
    for _, _, _, anchors in tiny["heads"]:
        tr = [min(w, a) * min(h, b) / (w * h + a * b - min(w, a) * min(h, b)) for a, b in anchors]
        differs |= tr.index(max(tr)) != R.fit_anchor(w, h, anchors)
    assert differs
    if len(g["tie_wh"]):
        w, h = g["tie_wh"].tolist()
        tied = False
        for _, _, _, anchors in tiny["heads"]:
            v = [min(w, a) * min(h, a) / (w * h + a * a - min(w, a) * min(h, a)) for a, _ in anchors]
            if v.count(max(v)) > 1:
                tied = True
                assert R.fit_anchor(w, h, anchors) == v.index(max(v))
        assert tied


def test_loss_ref_against_every_fixture_case(golden):
    for c in golden[1]:
        target, mask, n_obj, status = R.dense_targets(c["images"], c["heads"], 85)
        assert status == 0 and int(n_obj.sum()) == len(c["rows"]), c["name"]
        check_targets(c, target, mask, c["name"])
        comp, terms = R.components(c["pred"], target, mask)
        for q in range(5):                                            # float64 components: the reference's own, within the summation bound
            bound = R.sum_bound(c["comp64"][q], terms[q])
            if q == 1:                                                # tw / th may sit log_ulps away from the reference's
                m = np.asarray(mask)
                d = np.abs(c["pred"][m][:, 2:4].astype(np.float64) - target[m][:, 2:4].astype(np.float64))
                bound += float((10.0 * d * int(c["log_ulps"]) * np.spacing(np.abs(target[m][:, 2:4])).astype(np.float64)).sum())
            assert abs(comp[1 + q] - c["comp64"][q]) <= bound, (c["name"], R.NAMES[q], comp[1 + q], c["comp64"][q])
        assert abs(comp[0] - c["loss64"]) <= R.sum_bound(c["loss64"], sum(terms)) + 1e-300, c["name"]
        # the reference's own float32 sum: any order of float32 additions of n non-negative terms stays within n 2^-24 relative
        assert abs(comp[0] - float(c["loss32"])) <= sum(terms) * 2.0 ** -24 * comp[0], c["name"]


def _stub_model(text, height=416, width=None):
    return types.SimpleNamespace(blocks=parse_cfg_text(text), net_info={"height": height}, input_width=width)


def test_trainer_heads_come_from_the_cfg(golden):
    cases = golden[1]
    for text, c in ((cfgs.yolov3_tiny_cfg(416, 416), cases[0]), (cfgs.yolov3_cfg(416, 416), cases[3])):
        heads, classes = model_heads(_stub_model(text))
        assert classes == 80 and heads == c["heads"]
    heads, _ = model_heads(_stub_model(cfgs.mini_cfg(64, 160), 64, 160))                # rectangular: grid_h and grid_w differ
    assert [(h[0], h[1], h[2]) for h in heads] == [(2, 5, 32), (4, 10, 16)]
    arr = make_heads(heads)
    assert (arr[1].grid_h, arr[1].grid_w, arr[1].stride, arr[1].n_anchors) == (4, 10, 16, 3)
    assert list(arr[0].anchors[:6]) == [v for a in heads[0][3] for v in a]
    with pytest.raises(ValueError, match="at most 8"):
        make_heads([(1, 1, 32, [(10, 10)] * 9)])
    t = DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416)))
    assert (t.resolution, t.num_classes, t.TINY, t.min_box_size) == (416, 80, True, 24) and t.criterion == t.darknet_loss
    assert DarknetTrainer(_stub_model(cfgs.yolov3_cfg(416, 416))).TINY is False
    with pytest.raises(ValueError, match="num_classes"):
        DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416)), num_classes=3)


def test_trainer_host_mirrors_against_the_fixture(golden):
    g, cases = golden
    for c in cases:
        t = DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416) if c["N"] == 2535 else cfgs.yolov3_cfg(416, 416)))
        for (w, h), fit in zip(g["probe_wh"].tolist(), g["probe_fit"].tolist()):
            assert DarknetTrainer.anchor_fit(torch.tensor([0, 0, w, h]), cases[0]["heads"][0][3]) == fit
        layers, masks = [], []
        for im in c["images"]:
            per = [t.target_layer(torch.from_numpy(im), gh, anchors) for gh, _, _, anchors in c["heads"]]
            assert all(o.dtype == torch.float32 and m.dtype == torch.float32 and tuple(m.shape) == tuple(o.shape[:-1]) for o, m in per)
            layers.append(torch.cat([o for o, _ in per]))
            masks.append(torch.cat([m for _, m in per]))
        check_targets(c, torch.stack(layers).numpy(), torch.stack(masks).numpy() != 0, c["name"])
    t = DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416)))
    out, mask = t.target_layer(torch.from_numpy(np.asarray([_box(416, 100, 50, 50), _box(100, -1, 50, 50), _box(100, 416, 50, 50)])), 13, [(81, 82)])
    assert not out.any() and not mask.any()                           # outside the grid: skipped


def _box(cx, cy, w, h, cls=0, C_=80):
    r = np.zeros(5 + C_, F)
    r[:5] = (cx, cy, w, h, 1)
    r[5 + cls] = 1
    return r


def test_workspace_sizes_and_bad_arguments():
    lib = _ffi.lib()
    need = C.c_size_t()
    assert lib.rtod_yolo_loss_workspace(2, 2535, C.byref(need)) == 0
    assert need.value == (2 * 3 * 5 * 8 + 2 * 2535 * 4 + 15) // 16 * 16                 # partials of 3 workgroups per image + the owner map
    for bad in ((0, 10), (1, 0), (1 << 16, 1 << 16)):
        assert lib.rtod_yolo_loss_workspace(*bad, C.byref(need)) == -1 and "yolo_loss_workspace" in _ffi.last_error()
    assert lib.rtod_yolo_loss_workspace(1, 10, None) == -1


def _yolo_loss(**over):
    heads = over.pop("heads", [(2, 2, 32, [(10, 13), (16, 30)]), (4, 4, 16, [(33, 23)])])
    a = dict(pred=4096, batch=2, n_rows=24, num_class=3, n_heads=len(heads) if heads is not None else 1, boxes=4096, offs=4096, min_box=24.0, loss=4096, per_image=None,
             target=None, mask=None, n_obj=None, status=4096, ws=4096, ws_bytes=1 << 20)
    a.update(over)
    p = lambda v: None if v is None else C.c_void_p(v)
    return _ffi.lib().rtod_yolo_loss(p(a["pred"]), a["batch"], a["n_rows"], a["num_class"], make_heads(heads) if heads is not None else None, a["n_heads"],
                                     p(a["boxes"]), p(a["offs"]), a["min_box"], p(a["loss"]), p(a["per_image"]), p(a["target"]), p(a["mask"]), p(a["n_obj"]),
                                     p(a["status"]), p(a["ws"]), a["ws_bytes"], None)


@pytest.mark.parametrize("over,word", [
    (dict(pred=None), "null"), (dict(boxes=None), "null"), (dict(offs=None), "null"), (dict(loss=None), "null"), (dict(status=None), "null"),
    (dict(ws=None), "null"), (dict(heads=None, n_heads=1), "null"),
    (dict(batch=0), "batch"), (dict(num_class=0), "num_class"), (dict(n_rows=25), "n_rows is 25"), (dict(n_rows=23), "n_rows is 23"),
    (dict(n_heads=0), "heads outside"), (dict(n_heads=5), "heads outside"),
    (dict(heads=[(2, 2, 32, [(10, 13)] * 5)]), "n_rows is 24"), (dict(heads=[(0, 2, 32, [(10, 13)])]), "head 0"), (dict(heads=[(2, 2, 0, [(10, 13)])]), "head 0"),
    (dict(heads=[(2, 2, 32, [(10, 0)])]), "anchor"), (dict(heads=[(2, 2, 32, [])]), "head 0"),
    (dict(min_box=float("nan")), "not a number"), (dict(ws_bytes=100), "too small"), (dict(ws=4100), "aligned"),
])
def test_yolo_loss_refuses_bad_arguments_on_the_host(over, word):
    assert _yolo_loss(**over) == -1
    assert word in _ffi.last_error() and "yolo_loss" in _ffi.last_error()


@pytest.mark.parametrize("over,word", [
    (dict(pred=None), "null"), (dict(target=None), "null"), (dict(mask=None), "null"), (dict(loss=None), "null"), (dict(ws=None), "null"),
    (dict(rows=0), "rows"), (dict(attrs=4), "attrs"), (dict(attrs=0), "attrs"), (dict(ws_bytes=39), "too small"), (dict(ws=4100), "aligned"),
])
def test_darknet_loss_dense_refuses_bad_arguments_on_the_host(over, word):
    a = dict(pred=4096, target=4096, mask=4096, rows=100, attrs=85, loss=4096, ws=4096, ws_bytes=40)
    a.update(over)
    p = lambda v: None if v is None else C.c_void_p(v)
    rc = _ffi.lib().rtod_darknet_loss_dense(p(a["pred"]), p(a["target"]), p(a["mask"]), a["rows"], a["attrs"], p(a["loss"]), p(a["ws"]), a["ws_bytes"], None)
    assert rc == -1 and word in _ffi.last_error() and "darknet_loss_dense" in _ffi.last_error()


def test_finish_decode_refuses_a_null_plan():
    assert _ffi.lib().rtod_plan_finish_decode(None, C.c_void_p(4096), 1, None) == -1 and "finish_decode" in _ffi.last_error()


def test_trainer_has_no_cpu_path():
    t = DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416)))
    pred, tgt, mask = torch.zeros(1, 2535, 85), torch.zeros(1, 2535, 85), torch.zeros(1, 2535, dtype=torch.bool)
    for call in (lambda: t.loss_from_boxes(pred, [[]]), lambda: t.darknet_loss(pred, tgt, mask), lambda: t.criterion(pred, tgt, mask)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_cli_usage_names_the_loss_switch():
    from realtimeobjectdetection_amd import __main__ as M
    with pytest.raises(SystemExit) as e:
        M.main(["train"])
    assert "--loss" in str(e.value) and "out of scope" in str(e.value)
