"""GPU tests of rectangular network inputs (Darknet.input_width / rtod_plan_create_rect, rtod_prep_frames).  Run on an MI355X
with ``pytest -m gpu``.

The reference only defines the square network; the CPU reference here is tests/rect_ref.py (the oracle's trunk ops with the
head decode generalised to GH x GW, checked against RefDarknet.forward on squares by tests/test_rect_host.py).  Gates: those of
the square tests — fp32 / f16s3 output |got - ref| / max(1, |ref|) <= 1e-4 (test_gpu_parity.TOL), every materialised layer
within 2e-5 of its absmax (test_per_layer_vs_oracle), plain f16 p99.9 <= 5e-3 and max <= 2e-2 (test_f16_gpu.py).
"""
import os

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import cfgs, synth
from oracle import darknet_ref as O
from oracle import prep_ref
from rect_ref import forward_rect, synth_frames_rect

pytestmark = pytest.mark.gpu

TOL = 1e-4
P999_GATE, MAX_GATE = 5e-3, 2e-2
NETS = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg, "v5s": cfgs.yolov5s_style_cfg,
        # 3 classes: 24-channel heads, which an unfused plan can materialise (intermediate tensors need C % 4 == 0)
        "yolov3-c3": lambda: cfgs.yolov3_cfg(classes=3), "yolov3-tiny-c3": lambda: cfgs.yolov3_tiny_cfg(classes=3)}


def rel_err(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


_refs = {}


def _ref(net, h, w):
    """RefDarknet for (h, w) with the synthetic weights (the weights do not depend on the input size)."""
    key = (net, h, w)
    if key not in _refs:
        ref = O.RefDarknet(NETS[net](), h, w)
        wts = synth.synth_weights(ref.ir)
        ref.load_weight_stream(wts)
        _refs.clear()
        _refs[key] = (ref, wts)
    return _refs[key]


def _model(net, h, w, precision, d, wts, rect=True, **attrs):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / (net + ".cfg")), NETS[net]()), True).eval()
    m.net_info["height"] = h
    if rect:
        m.input_width = w
    m.precision = precision
    for k, v in attrs.items():
        setattr(m, k, v)
    m.load_weight_stream(wts)
    return m


def _check_output(got, want, precision):
    e = rel_err(got, want)
    if precision == "f16":
        assert np.quantile(e, 0.999) <= P999_GATE and e.max() <= MAX_GATE, (np.quantile(e, 0.999), e.max())
    else:
        assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


def _check_layers(m, outs, B):
    checked = 0
    for D in m.plan_description()["layers"]:
        i = D["index"]
        if D["type"] == "yolo" or (D["type"] == "convolutional" and D["fused_into"] >= 0):
            continue
        got = m.read_layer(i, B).cpu().numpy()
        want = outs[i].numpy()
        assert got.shape == want.shape, i
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max()) / scale
        assert err <= 2e-5, f"layer {i} ({D['type']}): max err/absmax {err:.3e}"
        checked += 1
    return checked


# ------------------------------------------------------------------------------- whole output + per layer
@pytest.mark.parametrize("precision", ["fp32", "f16s3", "f16"])
@pytest.mark.parametrize("h,w", [(352, 608), (608, 352)])
def test_yolov3_rect_vs_reference(tmp_path_factory, precision, h, w):
    B = 2
    ref, wts = _ref("yolov3", h, w)
    x = torch.from_numpy(synth_frames_rect(B, h, w, seed=11))
    with torch.no_grad():
        want, outs = forward_rect(ref, x, keep_layers=True)
    per_layer = precision != "f16"           # plain f16 is held to its output gates (test_f16_gpu.py), not to 2e-5 per layer
    m = _model("yolov3", h, w, precision, tmp_path_factory.mktemp("r%s%d" % (precision, h)), wts, keep_all_layers=per_layer)
    with torch.no_grad():
        got = m(x.cuda())
    torch.cuda.synchronize()
    assert m.active_precision == precision and not m.overflowed()
    assert got.shape == want.shape == (B, 3 * ((h // 8) * (w // 8) + (h // 16) * (w // 16) + (h // 32) * (w // 32)), 85)
    _check_output(got.cpu().numpy(), want.numpy(), precision)
    if per_layer:
        assert _check_layers(m, outs, B) == 78
    assert m.num_classes == 80 and len(m.anchors) == 9


@pytest.mark.parametrize("net,precision,h,w,B", [("yolov3-tiny", "fp32", 352, 608, 3), ("yolov3-tiny", "fp32", 608, 352, 1),
                                                 ("v5s", "f16s3", 384, 640, 2), ("v5s", "fp32", 640, 384, 1)])
def test_other_graphs_rect_vs_reference(tmp_path_factory, net, precision, h, w, B):
    ref, wts = _ref(net, h, w)
    x = torch.from_numpy(synth_frames_rect(B, h, w, seed=12))
    with torch.no_grad():
        want, outs = forward_rect(ref, x, keep_layers=True)
    m = _model(net, h, w, precision, tmp_path_factory.mktemp("o" + net), wts, keep_all_layers=True)
    with torch.no_grad():
        got = m(x.cuda())
    assert m.active_precision == precision
    _check_output(got.cpu().numpy(), want.numpy(), precision)
    assert _check_layers(m, outs, B) > 0


def test_unfused_options_and_standalone_decode_on_rectangles(tmp_path_factory):
    """fp32 plans with the stand-alone decode, add, copy and pack kernels (fuse_decode / fuse_shortcut / zero_copy_concat /
    stem_kernel = 0; 3 classes as in test_unfused_plan_options_vs_oracle): the GH x GW decode kernel and the element-wise kernels
    on rectangular views, against the reference."""
    h, w, B = 256, 416, 2
    for net in ("yolov3-tiny-c3", "yolov3-c3"):
        ref, wts = _ref(net, h, w)
        x = torch.from_numpy(synth_frames_rect(B, h, w, seed=13))
        with torch.no_grad():
            want = forward_rect(ref, x)
        m = _model(net, h, w, "fp32", tmp_path_factory.mktemp("u" + net), wts,
                   options={"fuse_decode": 0, "fuse_shortcut": 0, "zero_copy_concat": 0, "stem_kernel": 0})
        with torch.no_grad():
            got = m(x.cuda())
        kinds = {li.kind for li in m.launch_infos()}
        assert {1, 5}.issubset(kinds), kinds                            # input pack, stand-alone decode
        _check_output(got.cpu().numpy(), want.numpy(), "fp32")
        del m


# ------------------------------------------------------------------------------- bit identity
def _forced_outputs(tmp_path_factory, net, h, w, B, variants, option_sets):
    ref, wts = _ref(net, h, w)
    x = torch.from_numpy(synth_frames_rect(B, h, w, seed=14)).cuda()
    base = None
    d = tmp_path_factory.mktemp("f%s%d" % (net, h))
    for v in [-1] + variants:
        m = _model(net, h, w, "f16s3", d, wts, autotune=v < 0)
        if v >= 0:
            m.options["force_f16s3_variant"] = v
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
        assert not m.overflowed()
        if base is None:
            base = y.clone()
            with torch.no_grad():
                _check_output(base.cpu().numpy(), forward_rect(ref, x.cpu()).numpy(), "f16s3")
        else:
            assert torch.equal(y, base), (net, h, w, v)
        del m
    for opts in option_sets:
        m = _model(net, h, w, "f16s3", d, wts, options=dict(opts))
        with torch.no_grad():
            y = m(x)
        assert torch.equal(y, base), (net, h, w, opts)
        del m
    return base


ALL_VARIANTS = list(range(12)) + list(range(50, 70)) + list(range(70, 78)) + list(range(90, 101)) + list(range(110, 115))


@pytest.mark.parametrize("h,w", [(256, 416), (416, 256)])
def test_every_tile_variant_gives_the_same_bits_yolov3_rect(tmp_path_factory, h, w):
    """The rectangular twin of test_every_tile_variant_gives_the_same_bits: every split-f16 tile of every family forced in turn,
    the fused stem on / off and the hosted pointwise conv on / off, landscape and portrait: the autotuned plan's bits."""
    _forced_outputs(tmp_path_factory, "yolov3", h, w, 2, ALL_VARIANTS,
                    [{"stem2_kernel": 0}, {"stem2_kernel": 1}, {"fuse_pointwise": 0}, {"stem2_kernel": 0, "fuse_pointwise": 0},
                     {"ring_kernel": 0, "patch_kernel": 0, "pwd_kernel": 0}])


@pytest.mark.parametrize("h,w", [(256, 416), (416, 256)])
def test_every_tile_variant_gives_the_same_bits_v5s_rect(tmp_path_factory, h, w):
    _forced_outputs(tmp_path_factory, "v5s", h, w, 3, ALL_VARIANTS, [{"fuse_pointwise": 0}, {"pwd_kernel": 0}])


def test_rect_frames_are_independent(tmp_path_factory):
    h, w = 352, 608
    ref, wts = _ref("yolov3", h, w)
    x = torch.from_numpy(synth_frames_rect(4, h, w, seed=15)).cuda()
    for precision in ("f16s3", "f16"):
        m = _model("yolov3", h, w, precision, tmp_path_factory.mktemp("ind" + precision), wts)
        with torch.no_grad():
            y4 = m(x).clone()
            for i in range(4):
                assert torch.equal(m(x[i:i + 1].contiguous()), y4[i:i + 1]), (precision, i)
        del m


def test_square_rect_plan_is_bit_identical_to_the_classic_plan(tmp_path_factory):
    res, B = 608, 1
    ref, wts = _ref("yolov3", res, res)
    x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
    for precision in ("f16s3", "fp32"):
        d = tmp_path_factory.mktemp("sq" + precision)
        outs = []
        for rect in (False, True):
            m = _model("yolov3", res, res, precision, d, wts, rect=rect)
            with torch.no_grad():
                outs.append(m(x).clone())
            outs.append(m.get_tiles(B) if precision != "fp32" else None)
            del m
        assert torch.equal(outs[0], outs[2]), precision
        _check_output(outs[0].cpu().numpy(), ref.forward(x.cpu()).numpy(), precision)


def test_square_and_rect_plans_autotuned_in_one_process(tmp_path_factory):
    """Autotune memoises tiles per layer shape process-wide: a square plan and a rectangular one tuned one after the other (and
    the rectangle's transpose) must each match their own reference."""
    shapes = [(416, 416), (256, 416), (416, 256), (416, 416)]
    for h, w in shapes:
        ref, wts = _ref("yolov3", h, w)
        x = torch.from_numpy(synth_frames_rect(2, h, w, seed=16))
        m = _model("yolov3", h, w, "f16s3", tmp_path_factory.mktemp("mix%d_%d" % (h, w)), wts, rect=h != w)
        with torch.no_grad():
            got = m(x.cuda())
            want = forward_rect(ref, x)
        _check_output(got.cpu().numpy(), want.numpy(), "f16s3")
        del m


def test_rect_make_graphed_replays_bit_identically(tmp_path_factory):
    from realtimeobjectdetection_amd.util import write_results_async
    h, w = 352, 608
    ref, wts = _ref("yolov3", h, w)
    m = _model("yolov3", h, w, "f16s3", tmp_path_factory.mktemp("graph"), wts)
    xs = [torch.from_numpy(synth_frames_rect(2, h, w, seed=20 + i)).cuda() for i in range(3)]
    with torch.no_grad():
        want = []
        for x in xs:
            y = m(x)
            r, c = write_results_async(y, 80, 0.6, 0.5, cap=4096)
            want.append((y.clone(), r.clone(), c.clone()))
    run = m.make_graphed(xs[0], post=lambda y: write_results_async(y, 80, 0.6, 0.5, cap=4096))
    for x, (wy, wr, wc) in zip(xs, want):
        y, (r, c) = run(x)
        torch.cuda.synchronize()
        assert torch.equal(y, wy) and torch.equal(c, wc)
        assert torch.equal(r[:int(c[0])], wr[:int(wc[0])])


def test_rect_input_shape_is_checked(tmp_path_factory):
    h, w = 352, 608
    _, wts = _ref("yolov3-tiny", h, w)
    m = _model("yolov3-tiny", h, w, "fp32", tmp_path_factory.mktemp("shape"), wts)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, w, h, device="cuda"))
    m.input_width = None
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, h, w, device="cuda"))
    m.input_width = w
    m.train()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, h, w, device="cuda"))


# ------------------------------------------------------------------------------- prep_frames / rescale
def _frames(B, fh, fw, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (B, fh // 8 + 1, fw // 8 + 1, 3)).astype(np.float32)
    up = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :fh, :fw]                      # smooth-ish content plus noise
    return np.clip(up + rng.normal(0, 20, up.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("fh,fw,size", [(720, 1280, (608, 352)), (1280, 720, (608, 352)), (480, 640, (352, 608)), (333, 500, (416, 256))])
def test_prep_frames_vs_oracle(fh, fw, size):
    """Every frame of the batch against oracle.prep_ref's letterbox_image(img, (w, h)) + prep_image, at
    test_prep_image_gpu_vs_oracle's gate (at most one uint8 step, on fewer than 0.2 % of the values)."""
    from realtimeobjectdetection_amd.util import prep_frames
    B = 3
    fr = _frames(B, fh, fw, 7)
    got = prep_frames(fr, size, mode="BGR").cpu().numpy()
    assert got.shape == (B, 3, size[1], size[0])
    for b in range(B):
        c = prep_ref.letterbox_image(fr[b], size)
        want = (c[:, :, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
        diff = np.abs(got[b] - want) * 255.0
        assert diff.max() <= 1.0 + 1e-3 and (diff > 0.5).mean() < 2e-3, (b, diff.max(), (diff > 0.5).mean())


def test_prep_frames_square_equals_prep_image():
    from realtimeobjectdetection_amd.util import prep_frames, prep_image
    fr = _frames(1, 480, 640, 9)
    for mode in ("BGR", "RGB"):
        a = prep_frames(fr, 416, mode=mode)
        b = prep_image(fr[0], 416, mode=mode)
        assert torch.equal(a, b), mode
    a = prep_image(fr[0], (608, 352))
    b = prep_frames(fr, (608, 352))
    assert torch.equal(a, b)


def test_rescale_boxes_rect_on_device():
    from realtimeobjectdetection_amd.util import rescale_boxes
    iw, ih, size = 1280, 720, (608, 352)
    s = min(size[0] / iw, size[1] / ih)
    px = np.array([[50.0, 60.0, 700.0, 500.0], [-100.0, -100.0, 2000.0, 2000.0]])
    rows = np.zeros((2, 8), np.float32)
    rows[:, 1:5] = px * s
    rows[:, [1, 3]] += (size[0] - s * iw) / 2
    rows[:, [2, 4]] += (size[1] - s * ih) / 2
    out = rescale_boxes(torch.from_numpy(rows).cuda(), torch.tensor([[iw, ih]], dtype=torch.float32), size).cpu().numpy()
    assert np.abs(out[0, 1:5] - px[0]).max() <= 1e-2
    assert np.array_equal(out[1, 1:5], np.array([0, 0, iw, ih], np.float32))


# ------------------------------------------------------------------------------- detector
def test_detector_rect_resolution_end_to_end(tmp_path):
    """Darknetv3Detector(resolution=(608, 352)) on synthetic 1280x720 frames: metrics.json in the pinned schema, detections equal
    oracle.write_results on the CPU reference's output of the same preprocessed batch (write_results gate of the end-to-end
    square test)."""
    import json
    from PIL import Image
    from metrics_schema import validate_metrics
    from detcompare import assert_detections_equivalent
    from realtimeobjectdetection_amd.detect import Darknetv3Detector
    from realtimeobjectdetection_amd.util import prep_frames
    h, w = 352, 608
    ref, wts = _ref("yolov3-tiny", h, w)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    fr = _frames(3, 720, 1280, 21)
    names = []
    for i in range(3):
        names.append("f%d.png" % i)
        Image.fromarray(fr[i]).save(str(img_dir / names[-1]))
    cfg_path = cfgs.write_cfg(str(tmp_path / "yolov3-tiny.cfg"), NETS["yolov3-tiny"]())
    wpath = synth.write_weights_file(str(tmp_path / "t.weights"), wts)
    det = Darknetv3Detector(str(img_dir), str(tmp_path / "out"), cfg_path, wpath, (w, h), 0.5, 0.4, batch_size=3, draw=True)
    metrics = det()
    on_disk = json.load(open(os.path.join(str(tmp_path / "out"), "metrics.json")))
    validate_metrics(on_disk, names, 80, 0.5)
    x = prep_frames(fr, (w, h), mode="RGB").cpu()
    with torch.no_grad():
        want = O.write_results(forward_rect(ref, x), 80, 0.5, 0.4)
    want = np.zeros((0, 8), np.float32) if isinstance(want, int) else want.numpy()
    got = [r for n in names if metrics[n] != 0 for r in metrics[n]]
    got = np.array(got, np.float32).reshape(-1, 8)
    assert_detections_equivalent(got, want, 0.5, 0.4, tol=TOL)
    for n in names:
        assert os.path.exists(os.path.join(str(tmp_path / "out"), "det_yolov3-tiny_" + n))
