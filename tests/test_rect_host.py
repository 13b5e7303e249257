"""CPU tests of rectangular network inputs (H != W): rtod_plan_create_rect's plan against the Python IR, its head-grid check,
its identity with rtod_plan_create on square inputs, the letterbox geometry of prep_frames / rescale_boxes against the oracle's
letterbox_image, and the CPU reference the GPU tests compare with.  No compute call is made on a device."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from oracle import darknet_ref as O
from oracle import prep_ref
from rect_ref import forward_rect, synth_frames_rect

NETS = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg, "v5s": cfgs.yolov5s_style_cfg}
RECTS = [(352, 608), (608, 352), (384, 640), (640, 384), (256, 416)]       # (height, width)


def _create(text, h, w, rect=True, max_batch=4):
    lib = _ffi.lib()
    p = C.c_void_p()
    t = text.encode()
    fn = lib.rtod_plan_create_rect if rect else lib.rtod_plan_create
    return fn(t, len(t), h, w, max_batch, 0, C.byref(p)), p


def _describe(p):
    lib = _ffi.lib()
    need = C.c_size_t()
    assert lib.rtod_plan_describe(p, None, 0, C.byref(need)) == 0
    buf = C.create_string_buffer(need.value)
    assert lib.rtod_plan_describe(p, buf, need.value, None) == 0
    return buf.value.decode()


def _launches(p):
    lib = _ffi.lib()
    info = _ffi.PlanInfo()
    assert lib.rtod_plan_get_info(p, C.byref(info)) == 0
    out = []
    for i in range(info.n_launches):
        li = _ffi.LaunchInfo()
        assert lib.rtod_plan_get_launch(p, i, C.byref(li)) == 0
        out.append(tuple(getattr(li, f) for f, _ in li._fields_))
    return info, out


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("h,w", RECTS)
def test_rect_plan_matches_python_ir(net, h, w):
    text = NETS[net]()
    rc, p = _create(text, h, w)
    assert rc == 0, _ffi.last_error()
    d = json.loads(_describe(p))
    ir = build_ir(parse_cfg_text(text), h, w)
    assert (d["height"], d["width"]) == (h, w)
    assert d["total_rows"] == ir.total_rows and d["n_weight_floats"] == ir.n_weights and d["conv_flops"] == ir.conv_flops
    for L, D in zip(ir.layers, d["layers"]):
        assert (L.hin, L.win, L.hout, L.wout, L.cout) == (D["hin"], D["win"], D["hout"], D["wout"], D["cout"]), L.index
        assert (L.rows, L.row_offset) == (D["rows"], D["row_offset"])
    heads = [D for D in d["layers"] if D["type"] == "yolo"]
    assert heads and all(D["hout"] != D["wout"] for D in heads)
    assert all(h // D["hout"] == w // D["wout"] for D in heads)               # one stride per head
    assert d["total_rows"] == sum(len(D["anchors"]) * D["hout"] * D["wout"] for D in heads)
    info, _ = _launches(p)
    assert (info.height, info.width, info.total_rows) == (h, w, ir.total_rows)
    _ffi.lib().rtod_plan_destroy(p)


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("res", [320, 416, 608])
def test_square_rect_plan_is_the_classic_plan(net, res):
    """create_rect(h, h) is create(h, h): same describe JSON, same launch list, in every precision the cfg allows."""
    text = NETS[net]()
    for prec in (0, 1, 2):
        plans = []
        for rect in (False, True):
            rc, p = _create(text, res, res, rect)
            assert rc == 0, _ffi.last_error()
            prc = _ffi.lib().rtod_plan_set_precision(p, prec)
            plans.append((p, prc))
        (a, ra), (b, rb) = plans
        assert ra == rb
        assert _describe(a) == _describe(b)
        assert _launches(a)[1] == _launches(b)[1]
        for p in (a, b):
            _ffi.lib().rtod_plan_destroy(p)


def test_rect_head_with_two_strides_is_refused():
    """608x600: the stride-32 head is 19x19 but 600 // 19 = 31 along x — no single stride, RTOD_E_CFG naming the layer."""
    rc, p = _create(cfgs.yolov3_cfg(), 608, 600)
    assert rc == -3
    msg = _ffi.last_error()
    assert "layer 82" in msg and "stride" in msg, msg
    rc, p = _create(cfgs.yolov3_tiny_cfg(), 416, 400)
    assert rc == -3 and "layer" in _ffi.last_error()


def test_square_entry_point_still_refuses_rectangles():
    rc, p = _create(cfgs.yolov3_tiny_cfg(), 416, 320, rect=False)
    assert rc == -1
    rc, p = _create(cfgs.yolov3_tiny_cfg(), 0, 320)
    assert rc == -1


def test_rect_plan_refuses_batch_statistics_bn():
    lib = _ffi.lib()
    rc, p = _create(cfgs.yolov3_tiny_cfg(), 352, 608)
    assert rc == 0
    assert lib.rtod_plan_set_option(p, b"bn_batch_stats", 1) == -1
    assert "rectangular" in _ffi.last_error()
    lib.rtod_plan_destroy(p)
    rc, p = _create(cfgs.yolov3_tiny_cfg(), 416, 416)
    assert rc == 0 and lib.rtod_plan_set_option(p, b"bn_batch_stats", 1) == 0
    lib.rtod_plan_destroy(p)


def test_transposed_inputs_give_transposed_launches():
    """The launch lists of 352x608 and 608x352 differ only by transposed shapes: the per-launch (hout, wout) of one is the
    other's (wout, hout) — the plan carries both axes through (the autotune key includes hin / win / pad too)."""
    _, la = _launches(_create(cfgs.yolov3_cfg(), 352, 608)[1])
    _, lb = _launches(_create(cfgs.yolov3_cfg(), 608, 352)[1])
    f = [n for n, _ in _ffi.LaunchInfo._fields_]
    ho, wo = f.index("hout"), f.index("wout")
    assert len(la) == len(lb)
    assert all(a[ho] == b[wo] and a[wo] == b[ho] for a, b in zip(la, lb))


# ---------------------------------------------------------------------------------------- letterbox geometry (host)
def _oracle_geometry(img_w, img_h, size, monkeypatch):
    """(new_w, new_h, off_x, off_y) where oracle.prep_ref.letterbox_image(img, (w, h)) places the resized image."""
    monkeypatch.setattr(prep_ref, "resize_cubic_u8", lambda img, nw, nh: np.zeros((nh, nw, 3), np.uint8))
    c = prep_ref.letterbox_image(np.zeros((img_h, img_w, 3), np.uint8), size)
    assert c.shape == (size[1], size[0], 3)
    ys, xs = np.nonzero(c[:, :, 0] == 0)
    return int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), int(xs.min()), int(ys.min())


@pytest.mark.parametrize("img_wh", [(1280, 720), (720, 1280), (640, 480), (1920, 1080), (333, 777), (608, 352), (1000, 1000)])
@pytest.mark.parametrize("size", [(608, 352), (352, 608), (416, 256), (640, 384), (608, 608)])
def test_letterbox_geometry_matches_oracle(img_wh, size, monkeypatch):
    from realtimeobjectdetection_amd.util import letterbox_geometry
    assert letterbox_geometry(img_wh[0], img_wh[1], size) == _oracle_geometry(img_wh[0], img_wh[1], size, monkeypatch)
    if size[0] == size[1]:
        assert letterbox_geometry(img_wh[0], img_wh[1], size[0]) == letterbox_geometry(img_wh[0], img_wh[1], size)


@pytest.mark.parametrize("img_wh,size", [((1280, 720), (608, 352)), ((720, 1280), (608, 352)), ((640, 480), (352, 608)),
                                         ((333, 777), (416, 256))])
def test_rescale_boxes_inverts_a_rectangular_letterbox(img_wh, size, monkeypatch):
    """rescale_boxes((w, h)) maps canvas boxes back to the image: the placed image's corners go to the image's corners, an
    interior box goes back to where it came from, and boxes over the grey bars are clamped to the image."""
    from realtimeobjectdetection_amd.util import rescale_boxes
    iw, ih = img_wh
    nw, nh, ox, oy = _oracle_geometry(iw, ih, size, monkeypatch)
    s = min(size[0] / iw, size[1] / ih)
    px = np.array([[0.1 * iw, 0.2 * ih, 0.6 * iw, 0.9 * ih], [0.0, 0.0, iw, ih]], np.float64)
    fx = px.copy()
    fx[:, [0, 2]] = px[:, [0, 2]] * s + (size[0] - s * iw) / 2
    fx[:, [1, 3]] = px[:, [1, 3]] * s + (size[1] - s * ih) / 2
    rows = np.zeros((4, 8), np.float32)
    rows[:2, 1:5] = fx
    rows[2, 1:5] = [ox - 50, oy - 50, ox + nw + 50, oy + nh + 50]            # reaches into the bars on every side
    rows[3, 1:5] = [ox, oy, ox + nw, oy + nh]                                # the placed image
    out = rescale_boxes(torch.from_numpy(rows), torch.tensor([[iw, ih]], dtype=torch.float32), size).numpy()
    assert np.abs(out[:2, 1:5] - px).max() <= 1e-3 * max(iw, ih)
    assert np.array_equal(out[2, 1:5], np.array([0, 0, iw, ih], np.float32))
    assert np.abs(out[3, 1:5] - [0, 0, iw, ih]).max() <= 1.0 / s + 1e-3           # int() truncation of the placed size
    assert (out[:, [1, 3]] >= 0).all() and (out[:, [1, 3]] <= iw).all() and (out[:, [2, 4]] >= 0).all() and (out[:, [2, 4]] <= ih).all()


def test_rescale_boxes_int_is_unchanged():
    from realtimeobjectdetection_amd.util import rescale_boxes
    rng = np.random.default_rng(3)
    rows = np.zeros((50, 8), np.float32)
    rows[:, 0] = rng.integers(0, 3, 50)
    rows[:, 1:5] = np.sort(rng.uniform(-20, 640, (50, 4)), 1)
    dims = torch.tensor([[1280, 720], [480, 640], [416, 416]], dtype=torch.float32)
    a = rescale_boxes(torch.from_numpy(rows), dims, 416)
    b = rescale_boxes(torch.from_numpy(rows), dims, (416, 416))
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-3)


def test_detector_resolution_parsing():
    from realtimeobjectdetection_amd.detect import parse_resolution
    assert parse_resolution(416) == (416, 416, False)
    assert parse_resolution([608, 352]) == (608, 352, True)
    assert parse_resolution((352, 608)) == (352, 608, True)
    for bad in ([608, 350], [32, 352], [608, 352, 3], (0, 64)):
        with pytest.raises(ValueError):
            parse_resolution(bad)


# ---------------------------------------------------------------------------------------- CPU reference
@pytest.mark.parametrize("net,res,B", [("yolov3-tiny", 416, 2), ("yolov3", 320, 1), ("v5s", 256, 1)])
def test_rect_reference_reproduces_the_oracle_on_squares(net, res, B):
    text = NETS[net]()
    ref = O.RefDarknet(text, res)
    ref.load_weight_stream(synth.synth_weights(ref.ir))
    x = torch.from_numpy(synth.synth_frames(B, res))
    with torch.no_grad():
        want = ref.forward(x)
        got = forward_rect(ref, x)
    assert torch.equal(got, want)


def test_rect_reference_row_order():
    """Rows r = (gy * GW + gx) * A + a: the decoded x centre of row r sits in column gx, y in row gy (train=False)."""
    from rect_ref import predict_transform_rect
    GH, GW, A, C_ = 3, 5, 2, 1
    raw = torch.zeros(1, A * (5 + C_), GH, GW)
    out = predict_transform_rect(raw, 96, [(10, 13), (16, 30)], C_)
    stride = 96 // GH
    assert out.shape == (1, GH * GW * A, 5 + C_)
    for gy in range(GH):
        for gx in range(GW):
            for a in range(A):
                r = (gy * GW + gx) * A + a
                assert float(out[0, r, 0]) == (0.5 + gx) * stride and float(out[0, r, 1]) == (0.5 + gy) * stride
    x = torch.from_numpy(synth_frames_rect(1, 64, 96, 7))
    assert x.shape == (1, 3, 64, 96)
