"""CPU tests of the plain-f16 precision mode (precision 2, Darknet.precision = "f16"): the C ABI accepts the mode where the split
layout can express the cfg, every conv launch of such a plan runs a kernel family that has an f16 instance, and the CPU
emulation the GPU tests compare against (tests/f16_emulation.py) is the oracle's graph when its rounding is switched off."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from oracle import darknet_ref as O
from f16_emulation import F16Emulation, folded_f16_weights, round_act

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOD_E_ARG, RTOD_E_CFG = -1, -3


def _plan(text, res, max_batch=8):
    lib = _ffi.lib()
    h = C.c_void_p()
    t = text.encode()
    rc = lib.rtod_plan_create(t, len(t), res, res, max_batch, 0, C.byref(h))
    assert rc == 0, _ffi.last_error()
    return h


# families with a plain-f16 instance: generic tiles (100 + [0, 12)), bandd tiles (150 + [11, 20)), 1x1 slab tiles (190 + [0, 11))
def _f16_capable(variant):
    return 100 <= variant < 112 or 161 <= variant < 170 or 190 <= variant < 201


def test_set_precision_2_on_yolov3_and_refusals():
    lib = _ffi.lib()
    h = _plan(cfgs.yolov3_cfg(), 416)
    assert lib.rtod_plan_set_precision(h, 2) == 0, _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 3) == RTOD_E_ARG
    assert lib.rtod_plan_set_precision(h, -1) == RTOD_E_ARG
    lib.rtod_plan_destroy(h)
    # yolov3-tiny (Cin = 16 layer, maxpool chain) is not expressible in the split layout: refused like f16s3
    h = _plan(cfgs.yolov3_tiny_cfg(), 416)
    assert lib.rtod_plan_set_precision(h, 2) == RTOD_E_CFG
    assert "f16" in _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 0) == 0
    lib.rtod_plan_destroy(h)
    # batch-statistics BatchNorm runs on the exact-fp32 kernels only
    h = _plan(cfgs.yolov3_cfg(), 416)
    assert lib.rtod_plan_set_option(h, b"bn_batch_stats", 1) == 0, _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 2) == RTOD_E_CFG and "bn_batch_stats" in _ffi.last_error()
    lib.rtod_plan_destroy(h)
    # ... and the other order: an f16 plan refuses the option (the plan stays as it was)
    h = _plan(cfgs.yolov3_cfg(), 416)
    assert lib.rtod_plan_set_precision(h, 2) == 0
    assert lib.rtod_plan_set_option(h, b"bn_batch_stats", 1) == RTOD_E_CFG
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("net,res", [("yolov3", 416), ("yolov3", 608), ("yolov5s", 320)])
@pytest.mark.parametrize("force", [-1, 72, 112, 150, 161, 164, 190, 4])
def test_every_conv_launch_of_an_f16_plan_runs_an_f16_family(net, res, force):
    """Heuristic tiles and forced variants of other families (ring 72, patch 112, conv_band 150) fall back to f16-capable tiles;
    no fused stem + layer 1 launch, no hosted pointwise conv; kernel names carry the EPI_F16 bit."""
    lib = _ffi.lib()
    text = cfgs.yolov5s_style_cfg() if net == "yolov5s" else cfgs.yolov3_cfg()
    h = _plan(text, res)
    if force >= 0:
        assert lib.rtod_plan_set_option(h, b"force_f16s3_variant", force) == 0, _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 2) == 0, _ffi.last_error()
    info = _ffi.PlanInfo()
    assert lib.rtod_plan_get_info(h, C.byref(info)) == 0
    n_conv = 0
    for i in range(info.n_launches):
        li = _ffi.LaunchInfo()
        assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
        buf = C.create_string_buffer(256)
        assert lib.rtod_plan_launch_kernel_name(h, i, buf, 256) == 0, _ffi.last_error()
        name = buf.value.decode()
        if li.kind == 7:                                                  # LK_STEM: the split stem (a valid f16 producer)
            assert li.layer == 0 and li.bytes_per_frame > 0
            continue
        if li.kind != 0:
            assert name == ""
            continue
        assert li.flops_per_frame > 0 and not li.fused_pointwise, (li.layer, li.variant)
        if li.layer == 0:                                                 # pack + exact-fp32 conv writing the split layout
            assert li.variant < 100
            continue
        n_conv += 1
        assert _f16_capable(li.variant), (li.layer, li.variant, _ffi.lib().rtod_conv_variant_name(li.variant))
        m = re.match(r"void rtod::(\w+)<([\d, ]+)>\(rtod::ConvArgs, int, int\)$", name)
        assert m, name
        args = [int(t) for t in m.group(2).split(",")]
        epi = args[5] if m.group(1) == "conv_bandd_f16s3_kernel" else args[-1]      # bandd: <BM, BN, NWM, NWN, MINW, EPI, DB, KG, MAXW>
        assert epi & 8 and (epi & 7) in (0, 1, 2), name
    assert n_conv > 50
    lib.rtod_plan_destroy(h)


def test_f16_plan_describes_the_split_layout_and_the_same_weights_as_f16s3():
    """Mode 2 reuses mode 1's arena, views and weight packing unchanged."""
    lib = _ffi.lib()
    descs, infos = [], []
    for mode in (1, 2):
        h = _plan(cfgs.yolov3_cfg(), 608, 8)
        assert lib.rtod_plan_set_precision(h, mode) == 0
        need = C.c_size_t()
        assert lib.rtod_plan_describe(h, None, 0, C.byref(need)) == 0
        b = C.create_string_buffer(need.value)
        assert lib.rtod_plan_describe(h, b, need.value, None) == 0
        d = json.loads(b.value.decode())
        info = _ffi.PlanInfo()
        assert lib.rtod_plan_get_info(h, C.byref(info)) == 0
        descs.append((d["arena_floats"], d["bufs"], [(L["buf"], L["coff"]) for L in d["layers"]]))
        infos.append(info.packed_weight_bytes)
        lib.rtod_plan_destroy(h)
    assert descs[0] == descs[1] and infos[0] == infos[1]


def test_emulation_without_rounding_is_the_oracle():
    ref = O.RefDarknet(cfgs.yolov3_cfg(), 160)
    ref.load_weight_stream(synth.synth_weights(ref.ir))
    x = torch.from_numpy(synth.synth_frames(2, 160, seed=5))
    emu = F16Emulation(ref)
    with torch.no_grad():
        y_ref, l_ref = ref.forward(x, keep_layers=True)
        y0, l0 = emu.forward(x, rounding=False, keep_layers=True)
        y1 = emu.forward(x)
    assert torch.equal(y0, y_ref)
    assert all(torch.equal(l0[i], l_ref[i]) for i in l_ref)
    # with rounding the result moves, by about the floor of profiles/f16_floor.json, not more
    e = (y1 - y_ref).abs() / y_ref.abs().clamp(min=1.0)
    assert 1e-5 < float(e.max()) < 5e-2


def test_emulation_rounding_pieces():
    # activations: f16 of 8x, saturated at the f16 range
    x = torch.tensor([1.0, 1.0 + 2.0 ** -12, 1e-6, 9000.0, -9000.0, 0.1])
    r = round_act(x)
    assert float(r[0]) == 1.0 and float(r[1]) == 1.0                     # 8 (1 + 2^-12) rounds to 8 (11-bit significand)
    assert float(r[3]) == 65504.0 / 8 and float(r[4]) == -65504.0 / 8
    assert abs(float(r[5]) - 0.1) < 0.1 * 2.0 ** -11
    # weights: the folded fp32 weight without rounding, within half an f16 ulp of the channel maximum's scale with it
    ref = O.RefDarknet(cfgs.yolov3_cfg(), 160)
    ref.load_weight_stream(synth.synth_weights(ref.ir))
    L = ref.ir.layers[1]
    w0, b0 = folded_f16_weights(ref.params[1], L, rounding=False)
    w1, b1 = folded_f16_weights(ref.params[1], L, rounding=True)
    assert torch.equal(b0, b1)
    mx = w0.abs().flatten(1).max(1).values.view(-1, 1, 1, 1)
    assert bool(((w1 - w0).abs() <= mx * 2.0 ** -11).all()) and not torch.equal(w0, w1)


def test_floor_file_is_committed_and_under_the_gates():
    """profiles/f16_floor.json (tools/f16_floor.py) sets the GPU gates: its output floor must sit below the issue's ceilings
    (p99.9 <= 5e-3, max <= 2e-2 relative to max(1, |ref|)) for those ceilings to stand."""
    d = json.load(open(os.path.join(ROOT, "profiles", "f16_floor.json")))
    for tag in ("yolov3_416_b2", "yolov3_608_b1"):
        c = d["cases"][tag]
        assert 0 < c["output"]["p999"] <= 5e-3 and 0 < c["output"]["max"] <= 2e-2
        assert all(v["rms_rel"] > 0 for v in c["layers"].values())


def test_detector_passes_precision_to_the_model(tmp_path):
    from realtimeobjectdetection_amd.detect import Darknetv3Detector
    from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
    cfg = cfgs.write_cfg(str(tmp_path / "t.cfg"), cfgs.yolov3_tiny_cfg())
    w = synth.write_weights_file(str(tmp_path / "t.weights"), synth.synth_weights(build_ir(parse_cfg_text(cfgs.yolov3_tiny_cfg()), 416)))
    m = Darknetv3Detector(str(tmp_path), str(tmp_path / "out"), cfg, w, 416, 0.5, 0.4, precision="f16").configure_darknet()
    assert m.precision == "f16" and not m.training
    m = Darknetv3Detector(str(tmp_path), str(tmp_path / "out"), cfg, w, 416, 0.5, 0.4).configure_darknet()
    assert m.precision == os.environ.get("RTOD_PRECISION", "auto")
