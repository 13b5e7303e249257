"""GPU tests of the 16-filter split-f16 stem and its fused 2x2 max-pool (plan options "stem_pool" / "fuse_stem_pool",
conv_stem16_f16s3.hip).  Run on an MI355X with ``pytest -m gpu``.

Gates are the existing ones, unchanged (tests/test_narrow_gpu.py, tests/test_gpu_parity.py, tests/test_f16_gpu.py):
* fused and stand-alone forms give the same bits;
* f16s3: every materialised layer within 2e-5 of the layer's abs-max, the output within 1e-4 * max(1, |ref|), detections
  under detcompare's defaults;
* f16: the layer-local emulation gate (GPU-vs-emulation rms-relative at most 1/4 of fp32-vs-emulation, every layer from the
  GPU's own stored inputs), on YOLOv3-tiny the golden-row ceilings p99.9 <= 5e-3, max <= 2e-2.

The small network is cfgs.stem_pool_mini_cfg.  At 40x56 batch 3 there are 1680 pooled pixels: 105 wave tiles of 16, so the
four-wave workgroups end in a ragged one, and pooled rows of 28 pixels are no multiple of 8 or 16, so tiles straddle row
ends, both image borders and frame boundaries (560 pooled pixels per frame = 35 tiles).  At 64x64 batch 1 rows are whole tiles.
Under keep_all_layers the plan runs the stand-alone form (layer 0 is materialised and checked); without it, the fused form.
"""
import os

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import cfgs, synth
from oracle import darknet_ref as O
from detcompare import assert_detections_equivalent
from f16_emulation import rel
from rect_ref import forward_rect, predict_transform_rect, synth_frames_rect
from test_narrow_gpu import _check_layer_local, _check_layers, _materialised, _np_det

pytestmark = pytest.mark.gpu

TOL, LAYER_TOL = 1e-4, 2e-5
P999_GATE, MAX_GATE = 5e-3, 2e-2
FUSED = {"narrow_cin": 1, "stem_pool": 1}
UNFUSED = {"narrow_cin": 1, "stem_pool": 1, "fuse_stem_pool": 0}
MINI_SHAPES = [(40, 56, 3), (64, 64, 1)]


def _model(cfg_text, h, w, precision, d, wts, options=FUSED, **attrs):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / "net.cfg"), cfg_text), True).eval()
    m.net_info["height"] = h
    if w != h:
        m.input_width = w
    m.precision = precision
    m.options = dict(options)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.load_weight_stream(wts)
    return m


_refs = {}


def _ref(tag, cfg_text, h, w):
    """Oracle with the synthetic weights for (h, w): built once per shape, never modified."""
    key = (tag, h, w)
    if key not in _refs:
        ref = O.RefDarknet(cfg_text, h, w) if h != w else O.RefDarknet(cfg_text, h)
        wts = synth.synth_weights(ref.ir)
        ref.load_weight_stream(wts)
        _refs[key] = (ref, wts)
    return _refs[key]


_mini_want = {}


def _mini(h, w, B):
    ref, wts = _ref("mini", cfgs.stem_pool_mini_cfg(h, w), h, w)
    x = torch.from_numpy(synth_frames_rect(B, h, w, seed=11))
    return ref, wts, x


def _mini_reference(h, w, B):
    if (h, w, B) not in _mini_want:
        ref, _, x = _mini(h, w, B)
        with torch.no_grad():
            _mini_want[(h, w, B)] = forward_rect(ref, x, keep_layers=True)
    return _mini_want[(h, w, B)]


def _fwd(m, x):
    with torch.no_grad():
        y = m(x).clone()
    torch.cuda.synchronize()
    return y


def _describe_form(m):
    """Layer 0's fused_into of the prepared plan: 1 = the fused form runs, -1 = the stand-alone stem and a live max-pool."""
    return m.plan_description()["layers"][0]["fused_into"]


def _layer_intact_after_forward(m, layer, B):
    """True when no buffer written after `layer`'s last reader shares its arena range (read_layer is then valid without keep_all_layers)."""
    d = m.plan_description()
    bufs = d["bufs"]
    b = bufs[d["layers"][layer]["buf"]]
    lo, hi = b["offset"], b["offset"] + b["floats_per_frame"] * B
    for i, o in enumerate(bufs):
        if i == d["layers"][layer]["buf"] or o["last"] <= b["last"]:
            continue
        if o["offset"] < hi and lo < o["offset"] + o["floats_per_frame"] * B:
            return False
    return True


# ------------------------------------------------------------------------------- 1. fused == stand-alone, bit for bit
@pytest.mark.parametrize("precision", ["f16s3", "f16"])
@pytest.mark.parametrize("h,w,B", MINI_SHAPES)
def test_fused_equals_stand_alone_bitwise(tmp_path_factory, precision, h, w, B):
    _, wts, x = _mini(h, w, B)
    x = x.cuda()
    d = tmp_path_factory.mktemp("fe")
    text = cfgs.stem_pool_mini_cfg(h, w)
    fused = _model(text, h, w, precision, d, wts, autotune=False)
    plain = _model(text, h, w, precision, d, wts, options=UNFUSED, autotune=False)
    keep = _model(text, h, w, precision, d, wts, autotune=False, keep_all_layers=True)
    yf, yp, yk = _fwd(fused, x), _fwd(plain, x), _fwd(keep, x)
    assert fused.active_precision == precision
    assert _describe_form(fused) == 1 and _describe_form(plain) == -1 and _describe_form(keep) == -1
    assert not fused.overflowed() and not plain.overflowed() and not keep.overflowed()
    assert torch.isfinite(yf).all()
    assert torch.equal(yf, yp) and torch.equal(yf, yk)
    # the pooled map itself: what the fused kernel wrote into layer 1's view against stem + maxpool_split_kernel
    assert _layer_intact_after_forward(fused, 1, B) and _layer_intact_after_forward(fused, 2, B)
    for layer in (1, 2):
        got, want = fused.read_layer(layer, B), keep.read_layer(layer, B)
        assert got.shape == want.shape and torch.isfinite(want).all()
        assert torch.equal(got, want), (layer, int((got != want).sum()), float((got - want).abs().max()))


# ------------------------------------------------------------------------------- 2. f16s3 against the oracle
@pytest.mark.parametrize("h,w,B", MINI_SHAPES)
def test_mini_f16s3_vs_oracle(tmp_path_factory, h, w, B):
    _, wts, x = _mini(h, w, B)
    want, outs = _mini_reference(h, w, B)
    d = tmp_path_factory.mktemp("mo")
    text = cfgs.stem_pool_mini_cfg(h, w)
    keep = _model(text, h, w, "f16s3", d, wts, keep_all_layers=True)
    yk = _fwd(keep, x.cuda())
    assert keep.active_precision == "f16s3" and not keep.overflowed() and _describe_form(keep) == -1
    assert yk.shape == want.shape == (B, (h // 8) * (w // 8) * 3, 8)
    assert _check_layers(keep, outs, B) == 4                 # stem, pool, the Cin = 16 conv, the 32-channel conv (6 blocks - head conv - yolo)
    fused = _model(text, h, w, "f16s3", d, wts)
    yf = _fwd(fused, x.cuda())
    assert _describe_form(fused) == 1 and not fused.overflowed()
    e = rel(yf.cpu().numpy(), want.numpy())
    assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


# ------------------------------------------------------------------------------- 3. f16: layer-local emulation gate
@pytest.mark.parametrize("h,w,B", MINI_SHAPES)
def test_mini_f16_matches_its_emulation_layer_by_layer(tmp_path_factory, monkeypatch, h, w, B):
    monkeypatch.setattr(O, "predict_transform", predict_transform_rect)
    ref, wts, x = _mini(h, w, B)
    m = _model(cfgs.stem_pool_mini_cfg(h, w), h, w, "f16", tmp_path_factory.mktemp("mf"), wts, keep_all_layers=True)
    y = _fwd(m, x.cuda())
    assert m.active_precision == "f16" and not m.overflowed()
    assert [D["index"] for D in _materialised(m)][:2] == [0, 1]          # the stem and its pool are among the gated layers
    _check_layer_local(m, ref, x, y, B, 4)


# ------------------------------------------------------------------------------- 4. YOLOv3-tiny
def _tiny(res, B):
    ref, wts = _ref("tiny", cfgs.yolov3_tiny_cfg(), res, res)
    return ref, wts, torch.from_numpy(synth.synth_frames(B, res))


@pytest.mark.parametrize("res,B", [(416, 1), (608, 2)])
def test_tiny_f16s3_golden_rows_and_detections(golden_dir, tmp_path_factory, res, B):
    from realtimeobjectdetection_amd.util import write_results
    g = np.load(os.path.join(golden_dir, f"fwd_yolov3-tiny_{res}_b{B}.npz"))
    ref, wts, x = _tiny(res, B)
    m = _model(cfgs.yolov3_tiny_cfg(), res, res, "f16s3", tmp_path_factory.mktemp("tg"), wts)
    with torch.no_grad():
        y = m(x.cuda())
        y_ref = ref.forward(x)
    assert y.shape == (B, int(g["n_rows"]), 85) and m.active_precision == "f16s3" and not m.overflowed()
    assert _describe_form(m) == 1
    e = rel(y[:, ::int(g["row_stride"]), :].cpu().numpy(), g["rows"])
    print("tiny f16s3 %d b%d golden rows: max %.3e" % (res, B, e.max()))
    assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"
    d, gd = _np_det(write_results(y, 80, 0.6, 0.5)), _np_det(O.write_results(y_ref, 80, 0.6, 0.5))
    assert len(gd) > 0
    assert_detections_equivalent(d, gd, 0.6, 0.5)


def test_tiny_f16s3_per_layer(golden_dir, tmp_path_factory):
    res, B = 416, 1
    g = np.load(os.path.join(golden_dir, f"fwd_yolov3-tiny_{res}_b{B}.npz"))
    ref, wts, x = _tiny(res, B)
    with torch.no_grad():
        _, outs = ref.forward(x, keep_layers=True)
    m = _model(cfgs.yolov3_tiny_cfg(), res, res, "f16s3", tmp_path_factory.mktemp("tl"), wts, keep_all_layers=True)
    with torch.no_grad():
        m(x.cuda())
    torch.cuda.synchronize()
    assert m.active_precision == "f16s3" and not m.overflowed() and _describe_form(m) == -1
    assert _check_layers(m, outs, B) == 20                                 # 24 - 2 head convs - 2 yolo; layer 0 from the new stem
    for D in _materialised(m):                                             # ... and the real reference's per-layer probes
        i = D["index"]
        flat = m.read_layer(i, B).cpu().numpy().reshape(-1)
        scale = max(1.0, float(np.abs(outs[i].numpy()).max()))
        ge = np.abs(flat[g["layer_sample_idx"][i]] - g["layer_samples"][i]).max() / scale
        assert ge <= LAYER_TOL, f"layer {i}: vs reference probes {ge:.3e}"


@pytest.mark.parametrize("res,B", [(416, 1), (608, 2)])
def test_tiny_f16_golden_rows(golden_dir, tmp_path_factory, res, B):
    g = np.load(os.path.join(golden_dir, f"fwd_yolov3-tiny_{res}_b{B}.npz"))
    _, wts, x = _tiny(res, B)
    m = _model(cfgs.yolov3_tiny_cfg(), res, res, "f16", tmp_path_factory.mktemp("tf"), wts)
    y = _fwd(m, x.cuda())
    assert y.shape == (B, int(g["n_rows"]), 85) and m.active_precision == "f16" and not m.overflowed() and _describe_form(m) == 1
    e = rel(y[:, ::int(g["row_stride"]), :].cpu().numpy(), g["rows"])
    print("tiny f16 %d b%d golden rows: p99.9 %.3e, max %.3e" % (res, B, np.quantile(e, 0.999), e.max()))
    assert np.quantile(e, 0.999) <= P999_GATE and e.max() <= MAX_GATE, (np.quantile(e, 0.999), e.max())


# ------------------------------------------------------------------------------- 5. frames, batches, graph replay
@pytest.mark.parametrize("precision", ["f16s3", "f16"])
def test_frames_are_independent_and_graph_replay_gives_the_same_bits(tmp_path_factory, precision):
    h, w, B = 40, 56, 3
    _, wts, x = _mini(h, w, B)
    x = x.cuda()
    m = _model(cfgs.stem_pool_mini_cfg(h, w), h, w, precision, tmp_path_factory.mktemp("fi"), wts)
    want = _fwd(m, x)
    assert _describe_form(m) == 1 and not m.overflowed()
    perm = torch.tensor([2, 0, 1], device="cuda")
    y1 = _fwd(m, x[1:2])
    yp = _fwd(m, x[perm].contiguous())
    assert torch.equal(y1[0], want[1])
    assert torch.equal(yp, want[perm])
    run = m.make_graphed(x)
    for xi, wy in ((x[perm].contiguous(), yp), (x, want)):
        y, _ = run(xi)
        torch.cuda.synchronize()
        assert torch.equal(y, wy)


# ------------------------------------------------------------------------------- 6. range flag
@pytest.mark.parametrize("precision", ["f16s3", "f16"])
def test_fused_stem_saturates_and_raises_the_range_flag(tmp_path_factory, precision):
    h, w, B = 64, 64, 1
    ref, wts, x = _mini(h, w, B)
    # layer 0 x 2^15, layer 2 / 2^15: the stem's activations leave the split-f16 range, everything after it stays at its usual scale
    big = synth.scale_conv_weights(ref.ir, wts, 32768.0, layers=[0])
    big = synth.scale_conv_weights(ref.ir, big, 1.0 / 32768.0, layers=[2])
    probe = O.RefDarknet(cfgs.stem_pool_mini_cfg(h, w), h)
    probe.load_weight_stream(big)
    with torch.no_grad():
        _, layers = probe.forward(x, keep_layers=True)
    assert float(layers[0].abs().max()) > 8188.0 and float(layers[1].abs().max()) > 8188.0
    m = _model(cfgs.stem_pool_mini_cfg(h, w), h, w, precision, tmp_path_factory.mktemp("ov"), big, overflow_check="off")
    y = _fwd(m, x.cuda())
    assert _describe_form(m) == 1
    assert torch.isfinite(y).all()                                      # saturated, not inf - inf
    assert m.overflowed()
    ok = _model(cfgs.stem_pool_mini_cfg(h, w), h, w, precision, tmp_path_factory.mktemp("ok"), wts, overflow_check="off")
    _fwd(ok, x.cuda())
    assert not ok.overflowed()
