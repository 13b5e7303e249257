"""GPU tests of the training-loss path: rtod_yolo_loss / rtod_darknet_loss_dense (csrc/loss.hip) against the fixture recorded from
the reference's train.py and against tests/loss_ref.py, rtod_plan_finish_decode against an eval-decode forward, and
DarknetValidator.validate_model(loss=True) on a small network.

Gates.  Rows, masks and counts are integers; target values are compared bit for bit (tw / th against float32(log(float64(q))),
which is what the kernel is specified to compute, and within the recorded ulp distance of the reference's own values).  A loss
component is a sum of n non-negative float64 terms accumulated in double, on the device and on the host in different orders:
each side is within (n - 1) 2^-53 relative of the exact sum, so they differ by at most 2 n 2^-53 relative
(loss_ref.sum_bound, computed from n in every test).

Dense variant: rtod_darknet_loss_dense walks the flat [rows, attrs] tensor in workgroups of 1024 rows, rtod_yolo_loss walks every
image in workgroups of 1024 rows; for ONE image the partition and therefore every bit is the same, for several images the
results agree within the bound above.  Both are tested."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import loss_ref as R
from loss_cases import bits, check_targets, load_cases, make_pred
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T, validate as V
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_cases(golden_dir)


def run(pred, images, heads, num_class, min_box=24, dense=True):
    """One rtod_yolo_loss call through train.yolo_loss_async; everything back on the host."""
    out = T.yolo_loss_async(torch.from_numpy(np.ascontiguousarray(pred, F)).cuda(), [torch.from_numpy(np.asarray(im, F).reshape(-1, 5 + num_class)) for im in images],
                            heads, num_class, min_box, dense=dense, per_image=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_components(got, pred, target, mask, tag):
    """The six doubles of a call against the float64 formula over the call's own dense target; per-image rows likewise."""
    want, terms = R.components(pred, target, mask)
    comp = got["components"]
    for q in range(5):
        assert abs(comp[1 + q] - want[1 + q]) <= R.sum_bound(want[1 + q], terms[q]), (tag, R.NAMES[q], comp[1 + q], want[1 + q])
    assert comp[0] == (((comp[1] + comp[2]) + comp[3]) + comp[4]) + comp[5], tag        # the terms in darknet_loss's order
    for b in range(len(pred)):
        wb, tb = R.components(pred[b:b + 1], target[b:b + 1], mask[b:b + 1])
        pi = got["per_image"][b]
        for q in range(5):
            assert abs(pi[1 + q] - wb[1 + q]) <= R.sum_bound(wb[1 + q], tb[q]), (tag, b, R.NAMES[q])
        assert pi[0] == (((pi[1] + pi[2]) + pi[3]) + pi[4]) + pi[5], (tag, b)
    return want, terms


def check_against_ref(got, pred, images, heads, num_class, min_box, tag, status=0):
    """A call against tests/loss_ref.py: integers exact, every target value bit for bit, components within the bound."""
    target, mask, n_obj, st = R.dense_targets(images, heads, 5 + num_class, min_box)
    assert st == status and int(got["status"][0]) == status, tag
    assert np.array_equal(got["mask"] != 0, mask) and np.array_equal(got["n_obj"], n_obj), tag
    assert np.array_equal(bits(got["target"]), bits(target)), tag
    check_components(got, pred, got["target"], mask, tag)


def test_every_fixture_case(golden):
    for c in golden[1]:
        got = run(c["pred"], c["images"], c["heads"], 80)
        assert int(got["status"][0]) == 0, c["name"]
        check_targets(c, got["target"], got["mask"] != 0, c["name"])                     # columns 0, 1, 4..: the reference's bits
        per = [int(((c["rows"] >= b * c["N"]) & (c["rows"] < (b + 1) * c["N"])).sum()) for b in range(c["B"])]
        assert got["n_obj"].tolist() == per, c["name"]
        ref_t, ref_m, _, _ = R.dense_targets(c["images"], c["heads"], 85)
        assert np.array_equal(bits(got["target"][..., 2:4]), bits(ref_t[..., 2:4])), c["name"]   # tw / th = float32(log(float64(q)))
        mask = got["mask"] != 0
        _, terms = check_components(got, c["pred"], got["target"], mask, c["name"])
        comp = got["components"]
        for q in range(5):                                            # ... and the reference's own float64 components
            bound = R.sum_bound(c["comp64"][q], terms[q])
            if q == 1:
                d = np.abs(c["pred"][mask][:, 2:4].astype(np.float64) - got["target"][mask][:, 2:4].astype(np.float64))
                bound += float((10.0 * d * int(c["log_ulps"]) * np.spacing(np.abs(got["target"][mask][:, 2:4])).astype(np.float64)).sum())
            assert abs(comp[1 + q] - c["comp64"][q]) <= bound, (c["name"], R.NAMES[q], comp[1 + q], c["comp64"][q])


def _box(rng, H, W, C_, cls0=0.8, lo=2.0, hi=None):
    r = np.zeros(5 + C_, F)
    hi = float(max(H, W)) if hi is None else hi
    r[:5] = (rng.uniform(0, W - 0.01), rng.uniform(0, H - 0.01), rng.uniform(lo, hi), rng.uniform(lo, hi), 1.0)
    r[5 + (0 if rng.random() < cls0 or C_ == 1 else int(rng.integers(1, C_)))] = 1.0
    return r


GEOMETRIES = {
    # name: (input H, input W, heads, classes, batch, min_box)
    "g1_g2_a1_a3_c1": (64, 64, [(1, 1, 64, [(40, 50)]), (2, 2, 32, [(10, 14), (23, 27), (37, 58)])], 1, 1, 4),
    "g3_g7_a5_a1_c3": (63, 63, [(3, 3, 21, [(5, 9), (12, 7), (20, 25), (33, 30), (60, 60)]), (7, 7, 9, [(8, 8)])], 3, 3, 4),     # N = 94
    "rect_2x5_4x10_c80": (64, 160, [(2, 5, 32, [(116, 90), (156, 198), (373, 326)]), (4, 10, 16, [(30, 61), (62, 45), (59, 119)])], 80, 3, 4),   # N = 150
    "four_heads_a8": (96, 96, [(1, 1, 96, [(9 * k + 4, 11 * k + 3) for k in range(1, 9)]), (2, 2, 48, [(20, 20)]), (3, 3, 32, [(15, 40), (40, 15)]), (6, 6, 16, [(8, 8), (16, 16), (24, 24)])], 3, 2, 0),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_odd_geometry_against_loss_ref(name):
    H, W, heads, C_, B, min_box = GEOMETRIES[name]
    rng = np.random.default_rng(sorted(GEOMETRIES).index(name) + 31)
    N = sum(R.head_rows(heads))
    pred = make_pred(900 + N, B, N, 5 + C_)
    images = [np.stack([_box(rng, H, W, C_) for _ in range(int(rng.integers(3, 40)))]) for _ in range(B)]
    images[0][1] = images[0][0]                                       # an exact duplicate
    got = run(pred, images, heads, C_, min_box)
    assert got["n_obj"].sum() > 0
    check_against_ref(got, pred, images, heads, C_, min_box, name)
    empty = run(pred, [np.zeros((0, 5 + C_), F)] * B, heads, C_, min_box)                # every image empty: only the no-object term
    check_against_ref(empty, pred, [np.zeros((0, 5 + C_), F)] * B, heads, C_, min_box, name)
    assert not empty["mask"].any() and not empty["target"].any() and empty["components"][1:4].tolist() == [0, 0, 0] and empty["components"][4] > 0


def _crowd(C_=3):
    """Image 0: 300 boxes that all land in one cell of every head, most of them on one anchor (the last writer must win under
    contention), with exact duplicates; image 1: a few ordinary boxes."""
    rng = np.random.default_rng(77)
    heads = [(2, 2, 32, [(10, 14), (23, 27), (37, 58)]), (7, 7, 9, [(8, 8), (30, 30)])]
    a = np.zeros((300, 5 + C_), F)
    a[:, 0] = rng.uniform(36.1, 44.9, 300)                            # cell (1, 1) of the 2-grid, (4, 4) of the 7-grid (63 / 7 = 9)
    a[:, 1] = rng.uniform(36.1, 44.9, 300)
    a[:, 2:4] = rng.uniform(30, 60, (300, 2))
    a[:, 4] = 1
    a[np.arange(300), 5 + (rng.random(300) < 0.1).astype(int)] = 1
    a[200:250] = a[100:150]
    b = np.stack([_box(rng, 63, 63, C_) for _ in range(5)])
    return heads, [a, b], C_


def test_last_writer_wins_under_contention_and_calls_repeat_bit_for_bit(golden):
    heads, images, C_ = _crowd()
    N = sum(R.head_rows(heads))
    pred = make_pred(5, 2, N, 5 + C_)
    got = run(pred, images, heads, C_, 4)
    check_against_ref(got, pred, images, heads, C_, 4, "crowd")
    assert 0 < got["n_obj"][0] <= 5                                   # 300 boxes, one cell per head
    again = run(pred, images, heads, C_, 4)
    for k in ("components", "per_image", "target", "mask", "n_obj"):
        assert got[k].tobytes() == again[k].tobytes(), k
    c = golden[1][2]                                                  # three images, three workgroups each
    one, two = run(c["pred"], c["images"], c["heads"], 80, dense=False), run(c["pred"], c["images"], c["heads"], 80, dense=False)
    assert one["components"].tobytes() == two["components"].tobytes() and one["per_image"].tobytes() == two["per_image"].tobytes()


def _guarded(shape, dtype, fill):
    """A tensor of ``shape`` inside a larger buffer whose 64 leading and trailing elements hold ``fill``."""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
    return buf, buf[64:64 + n].view(*shape)


def test_out_of_grid_boxes_are_skipped_and_nothing_is_written_outside_the_outputs():
    H, W, heads, C_, B, min_box = GEOMETRIES["rect_2x5_4x10_c80"]
    rng = np.random.default_rng(5)
    N = sum(R.head_rows(heads))
    pred = make_pred(77, B, N, 5 + C_)
    inside = [np.stack([_box(rng, H, W, C_, lo=8) for _ in range(6)]) for _ in range(B)]
    bad = np.stack([_box(rng, H, W, C_, lo=8) for _ in range(7)])
    bad[:, 5:] = 0
    bad[:, 5] = 1
    bad[:, :2] = [(W, 10), (10, H), (W + 500, 10), (-0.5, 10), (10, -3), (np.nan, 10), (1e30, -1e30)]
    mixed = [np.concatenate([inside[0][:3], bad[:4], inside[0][3:]]), inside[1], np.concatenate([bad[4:], inside[2]])]
    clean = run(pred, inside, heads, C_, min_box)
    check_against_ref(clean, pred, inside, heads, C_, min_box, "inside")
    got = run(pred, mixed, heads, C_, min_box)
    check_against_ref(got, pred, mixed, heads, C_, min_box, "mixed", status=1)
    for k in ("components", "per_image", "target", "mask", "n_obj"):
        assert got[k].tobytes() == clean[k].tobytes(), k                                 # the other boxes' results are unchanged
    # the same call on guarded buffers, through the C ABI
    dev_pred = torch.from_numpy(pred).cuda()
    boxes, offs = T.pack_boxes([torch.from_numpy(m) for m in mixed], 5 + C_, dev_pred.device)
    ws, nbytes = T._workspace(dev_pred.device, B, N)
    bufs = {"loss": _guarded((6,), torch.float64, -7.0), "per_image": _guarded((B, 6), torch.float64, -7.0), "target": _guarded((B, N, 5 + C_), torch.float32, -7.0),
            "mask": _guarded((B, N), torch.uint8, 99), "n_obj": _guarded((B,), torch.int32, -7), "status": _guarded((1,), torch.int32, -7)}
    bufs["status"][1].zero_()
    p = lambda k: C.c_void_p(bufs[k][1].data_ptr())
    _ffi.check(_ffi.lib().rtod_yolo_loss(C.c_void_p(dev_pred.data_ptr()), B, N, C_, T.make_heads(heads), len(heads), C.c_void_p(boxes.data_ptr()), C.c_void_p(offs.data_ptr()),
                                         float(min_box), p("loss"), p("per_image"), p("target"), p("mask"), p("n_obj"), p("status"), C.c_void_p(ws.data_ptr()), nbytes, None))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        fill = 99 if k == "mask" else -7
        assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), k
    assert bufs["loss"][1].cpu().numpy().tobytes() == got["components"].tobytes()
    assert bufs["target"][1].cpu().numpy().tobytes() == got["target"].tobytes() and int(bufs["status"][1].item()) == 1


def _stub_model(text, height=416, width=None):
    return types.SimpleNamespace(blocks=parse_cfg_text(text), net_info={"height": height}, input_width=width)


def test_trainer_dense_route_and_fused_route(golden):
    for c in (golden[1][0], golden[1][2]):                            # one image (same bits), three images (within the bound)
        t = T.DarknetTrainer(_stub_model(cfgs.yolov3_tiny_cfg(416, 416)))
        pred = torch.from_numpy(c["pred"]).cuda()
        bnd = [torch.from_numpy(im) for im in c["images"]]
        target, mask = t.target_creator(bnd)
        assert target.is_cuda and target.dtype == torch.float32 and mask.dtype == torch.bool and tuple(mask.shape) == (c["B"], c["N"])
        check_targets(c, target.cpu().numpy(), mask.cpu().numpy(), c["name"])
        loss, comp = t.loss_from_boxes(pred, bnd)
        assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and comp.dtype == torch.float64 and tuple(comp.shape) == (6,)
        dense = t.criterion(pred, target, mask)
        assert dense.is_cuda and dense.dim() == 0 and dense.dtype == torch.float32
        fused, via_dense = comp.cpu().numpy(), t.last_components.cpu().numpy()
        assert int(t.status.item()) == 0
        if c["B"] == 1:
            assert fused.tobytes() == via_dense.tobytes(), c["name"]
        _, terms = R.components(c["pred"], target.cpu().numpy(), mask.cpu().numpy())
        for q in range(5):
            assert abs(fused[1 + q] - via_dense[1 + q]) <= R.sum_bound(fused[1 + q], terms[q]), (c["name"], R.NAMES[q])
        assert float(loss) == float(np.float32(fused[0])) and abs(fused[0] - c["loss64"]) <= R.sum_bound(c["loss64"], sum(terms))
    # darknet_loss on tensors no target_creator made: targets everywhere, objects in every second row, two leading dimensions
    rng = np.random.RandomState(3)
    p, tg = rng.random_sample((3, 700, 9)).astype(F), rng.random_sample((3, 700, 9)).astype(F)
    m = (np.arange(2100).reshape(3, 700) % 2).astype(bool)
    t.criterion(torch.from_numpy(p).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(m).cuda())
    want, terms = R.components(p, tg, m)
    got = t.last_components.cpu().numpy()
    for q in range(5):
        assert abs(got[1 + q] - want[1 + q]) <= R.sum_bound(want[1 + q], terms[q]), R.NAMES[q]


# ------------------------------------------------------------------------------------------ finish-decode, validator
def _model(d, text, res, precision, width=None):
    from realtimeobjectdetection_amd.darknet import Darknet
    ir = build_ir(parse_cfg_text(text), res, width)
    m = Darknet(cfgs.write_cfg(str(d / "m.cfg"), text), True).eval()
    m.net_info["height"] = res
    if width is not None:
        m.input_width = width
    m.precision = precision
    m.load_weight_stream(synth.synth_weights(ir))
    return m


@pytest.mark.parametrize("name,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "f16", None), ("mini", "fp32", 160), ("mini", "f16s3", 160), ("fallback", "fp32", None)])
def test_finish_decode_equals_the_eval_decode_bit_for_bit(tmp_path, name, precision, width):
    res, B = 64, 2
    text = cfgs.mini_cfg(res, width or res) if name == "mini" else cfgs.mini_fallback_cfg(res, res)   # fallback: one stand-alone decode launch, one fused
    m = _model(tmp_path, text, res, precision, width)
    x = torch.from_numpy(np.random.default_rng(9).random((B, 3, res, width or res), dtype=np.float32)).cuda()
    with torch.no_grad():
        want = m(x)
        with m.train_mode():
            got = m(x)
        raw = got.clone()
        assert m.finish_decode(got) is got
    assert m.active_precision == precision
    assert not torch.equal(raw[..., :4], want[..., :4]) and torch.equal(raw[..., 4:], want[..., 4:])   # TRAIN=True really differs in 0-3 only
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    with pytest.raises(ValueError, match="finish_decode"):
        m.finish_decode(got[:, :-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.finish_decode(got.cpu())


def test_validate_model_with_loss(tmp_path, capsys):
    res, B = 64, 4
    text = cfgs.mini_cfg(res, res)
    m = _model(tmp_path, text, res, "fp32")
    x = torch.from_numpy(synth.synth_frames(B, res, seed=5)).cuda()
    rng = np.random.default_rng(4)
    targets = [torch.from_numpy(np.stack([_box(rng, res, res, 80, cls0=0.7, lo=3, hi=40) for _ in range(6)])) for _ in range(B)]
    heads, _ = T.model_heads(m)
    names = ["f%d" % b for b in range(B)]
    for bs in (2, 4):
        batches = [(names[i:i + bs], x[i:i + bs], targets[i:i + bs]) for i in range(0, B, bs)]
        kw = dict(confidence=0.001, nms_thresh=0.5, resolution=res, min_box_size=4)
        plain, with_loss = V.DarknetValidator(**kw), V.DarknetValidator(**kw)
        plain.validate_model(m, batches, CUDA=True)
        with_loss.validate_model(m, batches, CUDA=True, loss=True)
        assert with_loss.total_scores == plain.total_scores and plain.total_scores["people_num"] > 0
        assert plain.total_scores["tp"] + plain.total_scores["fp"] > 0
        assert not hasattr(plain, "loss") and with_loss.loss_status == 0
        want, bound = np.zeros(6), np.zeros(6)
        for i in range(0, B, bs):
            with torch.no_grad(), m.train_mode():
                y_train = m(x[i:i + bs]).cpu().numpy()
            tg, mk, _, st = R.dense_targets([t.numpy() for t in targets[i:i + bs]], heads, 85, 4)
            comp, terms = R.components(y_train, tg, mk)
            assert st == 0 and mk.any()
            want += comp
            bound[1:] += [R.sum_bound(comp[1 + q], terms[q]) for q in range(5)]
            bound[0] += R.sum_bound(comp[0], sum(terms))
        nb = B // bs
        got = with_loss.loss_components.numpy()
        assert got.dtype == np.float64 and isinstance(with_loss.loss, float) and with_loss.loss == got[0]
        for q in range(6):                                            # mean per batch; the sum over batches and the division round too
            assert abs(got[q] - want[q] / nb) <= bound[q] / nb + (nb + 2) * 2.0 ** -53 * abs(want[q] / nb), (bs, q, got[q], want[q] / nb)
    assert "Loss" in capsys.readouterr().out


def test_cli_validate_with_loss_prints_and_stores_it(tmp_path, golden_dir, capsys):
    """``validate params.json --synthetic-weights --loss`` on YOLOv3-tiny at 416 and the three-image COCO file of validate.npz."""
    import json
    import os
    from PIL import Image
    from realtimeobjectdetection_amd import __main__ as M
    ann = json.loads(bytes(np.load(os.path.join(golden_dir, "validate.npz"))["coco_json"]).decode())
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for im in ann["images"]:
        Image.new("RGB", (im["width"], im["height"]), (90, 120, 150)).save(str(imgs / im["file_name"]))
    (tmp_path / "ann.json").write_text(json.dumps(ann))
    params = {"detector_params": {"images_path": str(imgs), "destination_path": str(tmp_path / "det"), "yolo_version": 3,
                                  "cfg_file_path": str(tmp_path / "cfg" / "yolov3-tiny.cfg"), "weights_file_path": str(tmp_path / "w" / "tiny.weights"),
                                  "resolution": 416, "confidence": 0.6, "nms_threshold": 0.5, "CUDA": True, "use_torch_weights": False, "batch_size": 2},
              "training_params": {"valid_annot_dir": str(tmp_path / "ann.json"), "valid_img_dir": str(imgs)}}
    (tmp_path / "params.json").write_text(json.dumps(params))
    M.main(["validate", str(tmp_path / "params.json"), "--synthetic-weights", "--loss"])
    assert "Loss = " in capsys.readouterr().out
    stored = json.load(open(str(tmp_path / "det" / "total_scores.json")))
    comp = stored["loss_components"]
    assert stored["loss"] > 0 and list(comp) == ["total", "xy", "wh", "obj", "noobj", "cls"] and comp["total"] == stored["loss"]
    assert comp["noobj"] > 0 and comp["obj"] > 0                      # the file's two class-0 boxes of at least 24 pixels are objects
    assert set(stored) >= {"people_num", "tp", "fp", "fn"}
