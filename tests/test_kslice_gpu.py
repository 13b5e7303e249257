"""GPU tests of the K-sliced split-f16 convolutions (plan option "k_slices_split", conv_ks_f16s3.hip).  Run on an MI355X with
``pytest -m gpu``.

Gates are the existing ones, unchanged:
* f16s3: every materialised layer within 2e-5 of the layer's abs-max, the output within 1e-4 * max(1, |ref|)
  (tests/test_gpu_parity.py: test_per_layer_vs_oracle, TOL), detections under detcompare's defaults;
* f16: the layer-local emulation gate of tests/test_f16_gpu.py (tests/test_narrow_gpu.py: _check_layer_local).

The small network is cfgs.kslice_mini_cfg at 40x56 batch 3 (rectangular: the CPU reference is tests/rect_ref.py) and 64x64
batch 1.  Under the rule (slices of 2 / 4 / 9 K-chunks for 8+ / 16+ / 32+ chunks on maps of at most 52x52) it holds: a 3x3
stride-2 conv of 9 chunks (5 slices, the last of one chunk); two 3x3 stride-1 convs of 18 chunks (slices of 4, the last of 2),
one of them with a fused shortcut, both band layers without the option; a 1x1 conv with Cin 256, linear activation and 96
filters (no multiple of a tile width) that writes a route's concat slice; a 99-chunk and a 36-chunk conv on 9-chunk slices; a
head conv of 8 chunks with fused decode and a 1-chunk 1x1 conv that stay on their old kernels.  The sliced layers have
B H W = 1680, 420 and 105 pixels at 40x56 batch 3: a ragged M tail on every tile (64 and 128 rows), several workgroups along M
and N.  All tiles x both schedules of the family must give the same bits, and a frame the same bits in any batch.
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

TOL = 1e-4
KS_TILES = range(150, 156)                    # 150 + 2 * tile + schedule (0: slices inside the workgroup, 1: one workgroup per slice)
SLICED = [2, 3, 4, 6, 7, 9, 10]               # layers of kslice_mini_cfg the rule slices
MINI_SHAPES = [(40, 56, 3), (64, 64, 1)]


def _model(cfg_text, h, w, precision, d, wts, options=None, **attrs):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / "net.cfg"), cfg_text), True).eval()
    m.net_info["height"] = h
    if w != h:
        m.input_width = w
    m.precision = precision
    m.options = {"k_slices_split": 1}
    m.options.update(options or {})
    for k, v in attrs.items():
        setattr(m, k, v)
    m.load_weight_stream(wts)
    return m


_refs = {}


def _mini(h, w, B):
    """Oracle with the synthetic weights, and the frames, of one shape: built once."""
    key = (h, w)
    if key not in _refs:
        ref = O.RefDarknet(cfgs.kslice_mini_cfg(h, w), h, w) if h != w else O.RefDarknet(cfgs.kslice_mini_cfg(h, w), h)
        wts = synth.synth_weights(ref.ir)
        ref.load_weight_stream(wts)
        _refs[key] = (ref, wts)
    ref, wts = _refs[key]
    return ref, wts, torch.from_numpy(synth_frames_rect(B, h, w, seed=7))


def _sliced_variants(m):
    return {li.layer: li.variant - 100 for li in m.launch_infos() if li.kind == 0 and li.variant - 100 in KS_TILES}


# ------------------------------------------------------------------------------- 1. against the references
@pytest.mark.parametrize("h,w,B", MINI_SHAPES)
def test_kslice_mini_f16s3_vs_oracle(tmp_path_factory, h, w, B):
    ref, wts, x = _mini(h, w, B)
    with torch.no_grad():
        want, outs = forward_rect(ref, x, keep_layers=True)
    m = _model(cfgs.kslice_mini_cfg(h, w), h, w, "f16s3", tmp_path_factory.mktemp("km"), wts, keep_all_layers=True)
    with torch.no_grad():
        y = m(x.cuda())
    torch.cuda.synchronize()
    assert m.active_precision == "f16s3" and not m.overflowed()
    assert sorted(_sliced_variants(m)) == SLICED
    assert {D["index"]: D["k_slices"] for D in m.plan_description()["layers"] if "k_slices" in D} == {2: 5, 3: 5, 4: 5, 6: 5, 7: 4, 9: 11, 10: 4}
    assert y.shape == want.shape == (B, (h // 8) * (w // 8) * 3, 8)
    assert _check_layers(m, outs, B) == 10                  # 13 blocks - the shortcut conv - the head conv - yolo (route 8 is materialised)
    e = rel(y.cpu().numpy(), want.numpy())
    assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


@pytest.mark.parametrize("h,w,B", MINI_SHAPES)
def test_kslice_mini_f16_matches_its_emulation_layer_by_layer(tmp_path_factory, monkeypatch, h, w, B):
    # the emulation decodes heads with the oracle's square predict_transform; rect_ref's is the same arithmetic on a GH x GW grid
    monkeypatch.setattr(O, "predict_transform", predict_transform_rect)
    ref, wts, x = _mini(h, w, B)
    m = _model(cfgs.kslice_mini_cfg(h, w), h, w, "f16", tmp_path_factory.mktemp("kmf"), wts, keep_all_layers=True)
    with torch.no_grad():
        y = m(x.cuda())
    torch.cuda.synchronize()
    assert m.active_precision == "f16" and not m.overflowed()
    assert sorted(_sliced_variants(m)) == SLICED
    _check_layer_local(m, ref, x, y, B, 10)


# ------------------------------------------------------------------------------- 2. tiles, schedules, frames, graph replay
def _forward_with_layers(m, x, B):
    with torch.no_grad():
        y = m(x).clone()
    torch.cuda.synchronize()
    return y, {D["index"]: m.read_layer(D["index"], B).clone() for D in _materialised(m)}


@pytest.mark.parametrize("precision", ["f16s3", "f16"])
def test_every_tile_and_schedule_frames_and_graph_replay_give_the_same_bits(tmp_path_factory, precision):
    h, w, B = 40, 56, 3
    ref, wts, x = _mini(h, w, B)
    x = x.cuda()
    d = tmp_path_factory.mktemp("kt")
    cfg_text = cfgs.kslice_mini_cfg(h, w)
    m = _model(cfg_text, h, w, precision, d, wts, keep_all_layers=True)
    want, want_layers = _forward_with_layers(m, x, B)       # autotuned
    tiles = m.get_tiles(B)
    launch_layer = [li.layer for li in m.launch_infos()]
    assert sorted(launch_layer[i] for i, v in enumerate(tiles) if v in KS_TILES) == SLICED and not m.overflowed()
    for v in KS_TILES:                                       # every family id on every sliced layer, through a tile table
        f = _model(cfg_text, h, w, precision, d, wts, autotune=False, keep_all_layers=True)
        f.prepare(B, x.device)
        f.set_tiles(B, [v if t in KS_TILES else t for t in tiles])
        y, layers = _forward_with_layers(f, x, B)
        assert set(_sliced_variants(f).values()) == {v} and not f.overflowed()
        assert torch.equal(y, want), v
        for i, t in layers.items():
            assert torch.equal(t, want_layers[i]), (v, i)
        del f
    # the option force_f16s3_variant reaches the sliced layers too; frame i alone on one workgroup per slice == row i of the
    # batch on the in-workgroup schedule
    fa = _model(cfg_text, h, w, precision, d, wts, autotune=False, options={"force_f16s3_variant": 152})
    fb = _model(cfg_text, h, w, precision, d, wts, autotune=False, options={"force_f16s3_variant": 151})
    with torch.no_grad():
        ya = fa(x).clone()
        assert set(_sliced_variants(fa).values()) == {152}
        assert torch.equal(ya, want)
        for i in range(B):
            yi = fb(x[i:i + 1]).clone()
            assert torch.equal(yi[0], ya[i]), i
        assert set(_sliced_variants(fb).values()) == {151}
    assert not fa.overflowed() and not fb.overflowed()
    # k_slice_workgroups = 0: the in-workgroup schedule everywhere, the bits of the default
    f0 = _model(cfg_text, h, w, precision, d, wts, options={"k_slice_workgroups": 0})
    with torch.no_grad():
        y0 = f0(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(y0, want)
    assert all(v % 2 == 0 for v in f0.get_tiles(B) if v in KS_TILES) and all(v % 2 == 0 for v in _sliced_variants(f0).values())
    # a permuted batch, and a captured forward
    with torch.no_grad():
        perm = torch.tensor([2, 0, 1], device="cuda")
        yp = m(x[perm].contiguous()).clone()
    assert torch.equal(yp, want[perm])
    run = m.make_graphed(x)
    for xi, wy in ((x, want), (x[perm].contiguous(), yp)):
        y, _ = run(xi)
        torch.cuda.synchronize()
        assert torch.equal(y, wy)
    assert not m.overflowed()


# ------------------------------------------------------------------------------- 3. one full network
def test_yolov3_416_b2_f16s3_golden_rows_and_detections(golden_dir, tmp_path_factory):
    from realtimeobjectdetection_amd.util import write_results
    res, B = 416, 2
    g = np.load(os.path.join(golden_dir, f"fwd_yolov3_{res}_b{B}.npz"))
    ir = O.RefDarknet(cfgs.yolov3_cfg(), res).ir
    m = _model(cfgs.yolov3_cfg(), res, res, "f16s3", tmp_path_factory.mktemp("ky"), synth.synth_weights(ir))
    x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
    with torch.no_grad():
        y = m(x)
        det = write_results(y, 80, 0.6, 0.5)
    assert y.shape == (B, int(g["n_rows"]), 85) and m.active_precision == "f16s3" and not m.overflowed()
    assert len(_sliced_variants(m)) == 63                    # every conv of the 52x52 / 26x26 / 13x13 stages with K >= 256 but the heads
    e = rel(y[:, ::int(g["row_stride"]), :].cpu().numpy(), g["rows"])
    assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"
    gd = np.load(os.path.join(golden_dir, f"det_yolov3_{res}_b{B}.npz"))["det"]
    assert len(gd) > 0
    assert_detections_equivalent(_np_det(det), gd, 0.6, 0.5)
