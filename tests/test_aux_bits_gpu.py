"""GPU test that pins the bits of the helper kernels of csrc/aux_kernels.hip: bilinear and nearest upsample, stand-alone shortcut
add, channel copy, max-pool, and batch-statistics BatchNorm (statistics, normalise, normalise + pool).  Run on an MI355X with
``pytest -m gpu``.

These kernels share one accessor per activation format, one body per op and one statement of the BatchNorm constants; this module
shows that they still give the bits of the library as it stood BEFORE that: tests/golden/aux_bits.json, written once by
tools/dump_aux_bits.py (its "recorded_from" names the commit).  It is not regenerated: a change of these bits is a change of the
arithmetic and has to be argued as such.

Every case is one forward of a small cfg with autotune off and update_running_stats off; the record holds, per case, the SHA-256 of
the float32 bytes of read_layer(layer) for the layers named, where stated the range flag, and for the BatchNorm cases a digest of
the float64 (mean, variance) rtod_plan_bn_batch_stats returns for every BatchNorm layer.  A case whose plan Darknet.prepare
refuses is absent from the record by construction (the split-f16 / plain-f16 plans refuse fuse_shortcut = 0 by themselves: there the
stand-alone add runs under option keep_backbone_activations, which is recorded beside them); every case's keys must equal the
recorded ones, so nothing drops out silently.

Elementwise cases (module in eval mode, keep_all_layers):
* mini_fallback_cfg 64x64 B 3 fp32: layers 5 (bilinear upsample), 6 (add), 9 (copy), 10 and 11 (pool stride 2 and stride 1);
* mini_cfg 64x64 B 3, f16s3 and f16, with fuse_shortcut = 0 and again with keep_backbone_activations: both shortcuts and the
  upsample; f16s3 once more with beta of one channel of both operands of shortcut 4 moved so that their sum leaves the format's
  range in either direction: digest and overflowed();
* pool_train_mini_cfg(stem=32) 40x40 B 3, f16s3 and f16: pools 1, 3, 5, 7 (7: stride 1 on the odd 5x5 map), upsample 15;
* v5_style_mini_cfg 128x128 B 2, fp32 / f16s3 / f16: layers 8 and 10 (size-5 symmetric pools, 10 on a concat view), 16 (nearest).
BatchNorm cases (training mode): every BatchNorm conv's stored layer, every pool behind one, all statistics:
* bn_pool_mini_cfg 64x64 B 2 and 40x40 B 3: the narrow option set with keep_all_layers (stand-alone pools), the same with
  fuse_bn_pool = 0, the narrow option set WITHOUT keep_all_layers (normalise + pool in one kernel: the layers still intact in
  the arena), and the exact-fp32 plan.  The 96- and 24-filter convs alone take the one-stage statistics;
* mini_cfg 64x64 B 3, fp32 and f16s3 + bn_batch_split: shortcuts on the two-stage path, the 1024-channel conv (C / 4 == 256);
* RES96_CFG below, 64x64 B 2, both plans: a shortcut on the one-stage path.
"""
import ctypes as C
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aux_bits.json")
NARROW = {"narrow_cin": 1, "stem_pool": 1, "bn_batch_split": 1, "bn_split_narrow": 1}          # OPTS of test_bn_narrow_gpu.py
BACKBONE = {"keep_head_inputs": 1, "keep_backbone_activations": 1}
SPLIT_BN = {"bn_batch_split": 1}

# a shortcut in the normalise kernel of a conv whose 96 filters keep the statistics on one stage (256 % 24 != 0)
RES96_CFG = """[net]
batch=1
subdivisions=1
width=64
height=64
channels=3

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=96
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=96
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-2
activation=linear

[convolutional]
filters=24
size=1
stride=1
pad=1
activation=linear

[yolo]
mask = 0,1,2
anchors = 10,13,  16,30,  33,23,  30,61,  62,45,  59,119,  116,90,  156,198,  373,326
classes=3
num=9
jitter=.3
ignore_thresh = .5
truth_thresh = 1
random=1
"""


def _elementwise():
    out = {"fallback/fp32": dict(text=cfgs.mini_fallback_cfg(64, 64), res=64, B=3, precision="fp32", layers=(5, 6, 9, 10, 11))}
    for p in ("f16s3", "f16"):
        for tag, opts in (("unfused", {"fuse_shortcut": 0}), ("held", BACKBONE)):
            out["mini_%s/%s" % (tag, p)] = dict(text=cfgs.mini_cfg(64, 64), res=64, B=3, precision=p, options=opts, layers=(4, 8, 18))
        out["pool_train/%s" % p] = dict(text=cfgs.pool_train_mini_cfg(40, 40, stem=32), res=40, B=3, precision=p, layers=(1, 3, 5, 7, 15))
    for tag, opts in (("unfused", {"fuse_shortcut": 0}), ("held", BACKBONE)):
        out["mini_%s_saturated/f16s3" % tag] = dict(text=cfgs.mini_cfg(64, 64), res=64, B=3, precision="f16s3", options=opts, layers=(4, 8, 18),
                                                     saturate=True)
    for p in ("fp32", "f16s3", "f16"):
        out["v5/%s" % p] = dict(text=cfgs.v5_style_mini_cfg(128, 128), res=128, B=2, precision=p, layers=(8, 10, 16))
    return out


def _batchnorm():
    out = {}
    for res, B in ((64, 2), (40, 3)):
        text = cfgs.bn_pool_mini_cfg(res, res)
        for tag, p, opts, keep in (("narrow", "f16s3", NARROW, True), ("narrow_unfused", "f16s3", dict(NARROW, fuse_bn_pool=0), True),
                                   ("narrow_fused", "f16s3", NARROW, False), ("fp32", "fp32", {}, True)):
            out["bn_pool_%d_b%d/%s" % (res, B, tag)] = dict(text=text, res=res, B=B, precision=p, options=opts, keep_all_layers=keep, train=True)
    for tag, p, opts in (("fp32", "fp32", {}), ("split", "f16s3", SPLIT_BN)):
        out["bn_mini/%s" % tag] = dict(text=cfgs.mini_cfg(64, 64), res=64, B=3, precision=p, options=opts, train=True)
        out["bn_res96/%s" % tag] = dict(text=RES96_CFG, res=64, B=2, precision=p, options=opts, train=True)
    return out


CASES = dict(_elementwise(), **_batchnorm())


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _saturating(ir, wts):
    """Copy of the stream with beta of channel 3 (channel 5) of layers 1 and 3, the operands of mini_cfg's shortcut 4, at 5000 (-50000:
    -5000 behind the leaky slope): each inside the split format's range of 8188, their sum outside it."""
    out = wts.copy()
    for layer in (1, 3):
        start = synth.conv_weight_slices(ir)[layer][0] - 4 * ir.layers[layer].cout            # beta, gamma, mean, var, weights
        out[start + 3] = np.float32(5000.0)
        out[start + 5] = np.float32(-50000.0)
    return out


def _intact(desc, layer, B):
    """True when no buffer written after ``layer``'s last reader shares its arena range (test_bn_narrow_gpu.py's rule)."""
    bufs = desc["bufs"]
    bi = desc["layers"][layer]["buf"]
    if bi < 0:
        return False
    b = bufs[bi]
    lo, hi = b["offset"], b["offset"] + b["floats_per_frame"] * B
    return not any(i != bi and o["last"] > b["last"] and o["offset"] < hi and lo < o["offset"] + o["floats_per_frame"] * B for i, o in enumerate(bufs))


def run_case(name, d):
    """{key: digest or flag} of one case, or None when Darknet.prepare refuses its plan."""
    from realtimeobjectdetection_amd.darknet import Darknet
    c = CASES[name]
    res, B, train = c["res"], c["B"], c.get("train", False)
    ir = build_ir(parse_cfg_text(c["text"]), res)
    wts = synth.synth_weights(ir)
    if c.get("saturate"):
        wts = _saturating(ir, wts)
    m = Darknet(cfgs.write_cfg(os.path.join(str(d), "net.cfg"), c["text"]), True)
    if not train:
        m.eval()
    m.net_info["height"] = res
    m.precision = c["precision"]
    m.options = dict(c.get("options", {}))
    m.keep_all_layers = c.get("keep_all_layers", True)
    m.autotune = False
    m.update_running_stats = False
    m.load_weight_stream(wts)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=9)).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                      # the training-mode warning
        try:
            m.prepare(B, x.device)
        except RuntimeError as e:
            print("AUX %s: refused (%s)" % (name, e))
            return None
        assert m.active_precision == c["precision"], name
        with torch.no_grad():
            y = m(x)
    torch.cuda.synchronize()
    desc = m.plan_description()
    L = desc["layers"]
    out = {}
    if train:
        convs = [D["index"] for D in L if D["type"] == "convolutional" and D["bn"]]
        stored = {D["fused_into"] if D["fused_into"] >= 0 else D["index"] for D in (L[i] for i in convs)}
        layers = sorted(stored | {i + 1 for i in convs if L[i + 1]["type"] == "maxpool"})
        if not m.keep_all_layers:
            layers = [i for i in layers if not (L[i]["type"] == "convolutional" and L[i]["fused_into"] >= 0) and _intact(desc, i, B)]
            assert any(L[i]["type"] == "maxpool" and L[i - 1]["fused_into"] == i for i in layers), (name, layers)     # a fused pool's map
        lib = _ffi.lib()
        for i in convs:
            n = L[i]["cout"]
            st = np.empty((2, n), np.float64)
            _ffi.check(lib.rtod_plan_bn_batch_stats(m._plan, i, st[0].ctypes.data_as(C.c_void_p), st[1].ctypes.data_as(C.c_void_p), n, None))
            out["stats/%d" % i] = _sha(st)
    else:
        layers = c["layers"]
    for i in layers:
        out["layer/%d" % i] = _sha(m.read_layer(i, B).cpu().float().contiguous().numpy())
    out["overflowed"] = bool(m.overflowed()) if m.active_precision != "fp32" else False
    if not c.get("saturate"):                                                # (saturated maps reach the heads' exp: the output is not looked at)
        assert torch.isfinite(y).all() and not out["overflowed"], name
    return out


def _record():
    return json.load(open(RECORD))["digests"]


def test_the_record_holds_no_unknown_case():
    rec = _record()
    assert set(rec) <= set(CASES)
    assert all(rec[n]["overflowed"] == bool(CASES[n].get("saturate")) for n in rec)            # the saturated add raised the flag, nothing else did


@pytest.mark.parametrize("name", sorted(CASES))
def test_helper_kernels_have_the_recorded_bits(tmp_path, name):
    got, rec = run_case(name, tmp_path), _record()
    if got is None:
        assert name not in rec, (name, "recorded, now refused")
        return
    assert name in rec, (name, "prepared, but absent from the record")
    want = rec[name]
    print("AUX %s: %d keys %s" % (name, len(got), sorted(got)))
    assert sorted(got) == sorted(want), (name, "keys produced against keys recorded")
    bad = [k for k in sorted(got) if got[k] != want[k]]
    assert not bad, (name, "keys whose bits differ from the record", bad)
