"""GPU test that pins the float bits of the training path across commits: the weight gradients (csrc/wgrad.hip through
rtod_conv1x1_wgrad and rtod_conv_wgrad), the optimiser steps that re-pack in place (csrc/head_step.hip through
rtod_plan_step_conv and rtod_plan_step_conv_folded) and their host twins (rtod_plan_update_conv, rtod_plan_update_conv_weight).
Run on an MI355X with ``pytest -m gpu``.

The other GPU tests hold these kernels to integer exactness, to a summation bound, to the host pack and to call-to-call
reproducibility; none of that fixes the bits of a float sum from one commit to the next.  This file compares them with a record,
tests/golden/train_bits.json, written once by tools/dump_train_bits.py from the library as it stood BEFORE the head and block
entries were put on one code path (its "recorded_from" names the commit).  It is not regenerated: a change of these bits is a
change of the arithmetic, of the slice rule or of the summation order and has to be argued as such.

* Weight gradients: SHA-256 of the float32 bytes of dW and of db on shapes from head_grad_cases.py / block_grad_cases.py — one
  slice, the slice cap below 16 (524 tiles: cap 2, with a random float64 row scale), 16 slices with K one short of a slice
  boundary, Cout tails, chunks that cross an image boundary.  Inputs are seeded standard normals.
* Steps: mini_cfg(64, 64) with both keep options, trainable="blocks", on the batch of test_block_grad_gpu._batch(): one SGD step,
  then two Adam steps; after each phase the packed image, every master and every moment are hashed.
* Updates: update_conv / update_conv_weight of every trained conv with its master; the packed image keeps its hash.

A second record, tests/golden/grad_bits.json, holds the data gradients (csrc/dgrad.hip through rtod_conv1x1_dgrad, rtod_conv_dgrad and
rtod_conv_dgrad_s2) and the stride-2 weight gradient (rtod_conv_wgrad_s2) to the bits they had BEFORE their kernels were put on one
tile loop; the same dumper writes it (``--grad``) and it is not regenerated either.

* Data gradients: SHA-256 of dx on neck_grad_cases.DGRAD_SHAPES (1x1 entry; rtod_conv_dgrad sizes 1 and 3) and on
  backbone_grad_cases.S2_SHAPES (stride 2), plain and with the random signed float64 row scale of CAP_SHAPE above, with y given and
  slope 0.1; y is a standard normal with every 7th element set to 0.0, so the mask sees positives, negatives and exact zeros.  One
  further digest per size runs without y.
* Stride-2 weight gradients: dW and db on S2_SHAPES, and with the row scale on the ragged-Cout shape.

A third record, tests/golden/thin_bits.json (``--thin``), holds the thin-conv gradients (rtod_conv_wgrad_thin, rtod_conv_dgrad_thin) and
one walk of the "full" scope to the bits they had BEFORE the thin weight gradient was folded into the one launcher of csrc/wgrad.hip.

* Thin weight gradients: dW on full_grad_cases.WGRAD_THIN_SHAPES and on THIN_TREE_SHAPES, which a host mirror of the slice rule chose
  so that the reduction tree has a second level (more than 32 slices), a ragged last group and a short last slice, with the slice length
  on the lower clamp (256), strictly between the clamps (304) and on the upper one (1024); the test asserts these (slices, slice
  length) through conv_wgrad_thin_slices.  Two of them also run with the random signed float64 row scale.
* Thin data gradients: dx on full_grad_cases.DGRAD_THIN_SHAPES, plain and scaled, y and slope as above.
* One walk: DarknetTrainer.full_gradients on pool_train_mini_cfg(64, 64, classes=3, stem=16), fp32, on the batch of
  test_full_grad_gpu._batch: one digest per trained conv's dW (the Python routing, and layer 0 over the prepared network input).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import cfgs, train as T
from realtimeobjectdetection_amd.train import HeadOptimizer
from backbone_grad_cases import S2_SHAPES, out_hw
from full_grad_cases import DGRAD_THIN_SHAPES, POOL_MINI_FULL, WGRAD_THIN_SHAPES
from neck_grad_cases import DGRAD_SHAPES
from test_block_grad_gpu import _batch, _block_trainer
from test_full_grad_gpu import _batch as _full_batch, _full_trainer

pytestmark = pytest.mark.gpu
F = np.float32
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_bits.json")

HEAD_SHAPES = [(2, 18, 32, 2, 2), (3, 255, 96, 13, 13), (1, 64, 64, 127, 1)]      # (B, Cout, Cin, H, W)
CAP_SHAPE = (2, 256, 928, 4, 4)                                                    # size 3: 524 tiles, at most 2 slices
WGRAD_CASES = [("conv1x1_wgrad", 1, s) for s in HEAD_SHAPES] + [("conv_wgrad", size, s) for size in (1, 3) for s in HEAD_SHAPES + [CAP_SHAPE]]
PRECISIONS = ["fp32", "f16s3"]

GRAD_RECORD = os.path.join(os.path.dirname(RECORD), "grad_bits.json")
RAGGED = (3, 255, 96, 13, 13)                                                      # Cout 255, a Cin tail tile, tiles across images
# (entry, size, stride, shape, scaled, masked): stride 2 reads shape's H x W as the conv's INPUT map
GRAD_CASES = ([("conv1x1_dgrad", 1, 1, s, False, True) for s in DGRAD_SHAPES]
              + [("conv_dgrad", size, 1, s, scaled, True) for size in (1, 3) for s in DGRAD_SHAPES for scaled in (False, True)]
              + [("conv_dgrad", size, 1, RAGGED, False, False) for size in (1, 3)]
              + [("conv_dgrad", 3, 2, s, scaled, True) for s in S2_SHAPES for scaled in (False, True)]
              + [("conv_wgrad", 3, 2, s, False, False) for s in S2_SHAPES] + [("conv_wgrad", 3, 2, RAGGED, True, False)])

THIN_RECORD = os.path.join(os.path.dirname(RECORD), "thin_bits.json")
# (B, Cout, Cin, H, W, size) -> (slices, slice length) of rtod_conv_wgrad_thin.  66 slices: groups of 32 + 32 + 2, the last slice 130 terms;
# 72 slices on 2 x 2 tiles: 32 + 32 + 8; 8 tiles: L = 304 strictly between the clamps, the last slice 96 terms; one tile over
# K = 1,049,600: L on the upper clamp, 33 groups, the last of one slice
THIN_TREE_SHAPES = {(1, 16, 3, 129, 130, 3): (66, 256), (2, 40, 16, 96, 96, 3): (72, 256), (1, 97, 16, 160, 240, 3): (127, 304),
                    (1, 1, 1, 1025, 1024, 1): (1025, 1024)}
THIN_SCALED = [(1, 16, 3, 129, 130, 3), (1, 97, 16, 160, 240, 3)]
# (entry, shape, scaled)
THIN_CASES = ([("conv_wgrad_thin", s, False) for s in WGRAD_THIN_SHAPES + list(THIN_TREE_SHAPES)] + [("conv_wgrad_thin", s, True) for s in THIN_SCALED]
              + [("conv_dgrad_thin", s, scaled) for s in DGRAD_THIN_SHAPES for scaled in (False, True)])
THIN_WALK = "full_gradients/pool_train_mini_64x64_stem16/fp32"


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def wgrad_key(entry, size, shape):
    return "%s/size%d/%s" % (entry, size, "x".join(str(v) for v in shape))


def wgrad_digest(entry, size, shape):
    """{"dw", "db"}: digests of one weight-gradient call on seeded inputs."""
    B, cout, cin, H, W = shape
    rng = np.random.RandomState(1000 * B + 10 * cout + H * W + size)
    dz = torch.from_numpy(rng.standard_normal((B, cout, H, W)).astype(F)).cuda()
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(F)).cuda()
    if entry == "conv1x1_wgrad":
        dw, db = T.conv1x1_wgrad_async(dz, x)
    else:
        scale = torch.from_numpy(rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).cuda() if shape == CAP_SHAPE else None
        dw, db = T.conv_wgrad_async(dz, x, size, row_scale=scale, bias=True)
    assert tuple(dw.shape) == (cout, cin, size, size) and tuple(db.shape) == (cout,)
    return {"dw": sha(dw), "db": sha(db)}


def grad_key(entry, size, stride, shape, scaled, masked):
    return "%s/size%d/stride%d/%s/%s%s" % (entry, size, stride, "x".join(str(v) for v in shape), "scaled" if scaled else "plain",
                                           "" if masked or "wgrad" in entry else "/linear")


def grad_digest(entry, size, stride, shape, scaled, masked):
    """{"dx"} of one data-gradient call or {"dw", "db"} of one stride-2 weight-gradient call on seeded inputs."""
    B, cout, cin, H, W = shape
    Ho, Wo = out_hw(H, W) if stride == 2 else (H, W)
    rng = np.random.RandomState(1000 * B + 10 * cout + H * W + size + 7 * stride)
    w = torch.from_numpy(rng.standard_normal((cout, cin, size, size)).astype(F)).cuda()
    dz = torch.from_numpy(rng.standard_normal((B, cout, Ho, Wo)).astype(F)).cuda()
    y = rng.standard_normal((B, cin, H, W)).astype(F)                 # the conv's input map: y of a data gradient, x of a weight gradient
    scale = torch.from_numpy(rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).cuda() if scaled else None
    if entry == "conv_wgrad":
        dw, db = T.conv_wgrad_async(dz, torch.from_numpy(y).cuda(), size, row_scale=scale, bias=True, stride=stride)
        assert tuple(dw.shape) == (cout, cin, size, size) and tuple(db.shape) == (cout,)
        return {"dw": sha(dw), "db": sha(db)}
    y.reshape(-1)[::7] = 0.0                                          # exact zeros next to the negatives: the !(y > 0) branch
    y = torch.from_numpy(y).cuda() if masked else None
    if entry == "conv1x1_dgrad":
        dx = T.conv1x1_dgrad_async(w, dz, y=y, slope=0.1)
    else:
        dx = T.conv_dgrad_async(w, dz, size, row_scale=scale, y=y, slope=0.1, stride=stride, in_hw=(H, W))
    assert tuple(dx.shape) == (B, cin, H, W)
    return {"dx": sha(dx)}


def thin_key(entry, shape, scaled):
    return "%s/%s/%s" % (entry, "x".join(str(v) for v in shape), "scaled" if scaled else "plain")


def thin_digest(entry, shape, scaled):
    """{"dw"} of one thin weight-gradient call or {"dx"} of one thin data-gradient call on seeded inputs (grad_digest's y and slope)."""
    B, cout, cin, H, W, size = shape
    rng = np.random.RandomState(1000 * B + 10 * cout + H * W + size + cin)
    w = torch.from_numpy(rng.standard_normal((cout, cin, size, size)).astype(F)).cuda()
    dz = torch.from_numpy(rng.standard_normal((B, cout, H, W)).astype(F)).cuda()
    y = rng.standard_normal((B, cin, H, W)).astype(F)
    scale = torch.from_numpy(rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).cuda() if scaled else None
    if entry == "conv_wgrad_thin":
        dw = T.conv_wgrad_thin_async(dz, torch.from_numpy(y).cuda(), size, row_scale=scale)
        assert tuple(dw.shape) == (cout, cin, size, size)
        return {"dw": sha(dw)}
    y.reshape(-1)[::7] = 0.0
    dx = T.conv_dgrad_thin_async(w, dz, size, row_scale=scale, y=torch.from_numpy(y).cuda(), slope=0.1)
    assert tuple(dx.shape) == (B, cin, H, W)
    return {"dx": sha(dx)}


def walk_digest(d):
    """{conv: digest of its dW} of one full_gradients walk of pool_train_mini_cfg(64, 64, classes=3, stem=16), fp32."""
    m, t = _full_trainer(d, 64, 64, "fp32", 16)
    xd, bnd = _full_batch(64, 64)
    _, _, grads = t.full_gradients(xd, bnd)
    assert m.active_precision == "fp32" and sorted(grads) == POOL_MINI_FULL[16]
    return {str(c): sha(dw) for c, dw in sorted(grads.items())}


def _state_digest(m, t):
    out = {"image": sha(m.packed_weights())}
    for layer, st in sorted(t.optimizer.state.items()):
        for k, v in sorted(st.items()):
            out["%d.%s" % (layer, k)] = sha(v) if isinstance(v, torch.Tensor) else int(v)
    return out


def step_digest(precision, d):
    """{"sgd", "adam", "update"}: digests of the packed image, the masters and the moments after one SGD step, after two further
    Adam steps, and of the image after the host twins re-packed every trained conv from its master."""
    m, t = _block_trainer(d, cfgs.mini_cfg(64, 64), 64, precision)
    xd, bnd = _batch()
    out = {}
    t.optimizer = HeadOptimizer("sgd", lr=1e-4)
    t.feed_forward_through_model(xd, bnd)
    out["sgd"] = _state_digest(m, t)
    t.optimizer = HeadOptimizer("adam", lr=1e-4)
    for _ in range(2):
        t.feed_forward_through_model(xd, bnd)
    out["adam"] = _state_digest(m, t)
    assert m.active_precision == precision and sorted(t._head_masters) == [13, 14, 21, 22]
    for layer, (w, b) in sorted(t._head_masters.items()):
        if b is None:
            m.update_conv_weight(layer, w)
        else:
            m.update_conv(layer, w, b)
    out["update"] = {"image": sha(m.packed_weights())}
    return out


def _record(path=RECORD):
    with open(path) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("entry,size,shape", WGRAD_CASES)
def test_weight_gradient_has_the_recorded_bits(entry, size, shape):
    got = wgrad_digest(entry, size, shape)
    print("TRAIN BITS %s: %s" % (wgrad_key(entry, size, shape), got))
    assert got == _record()[wgrad_key(entry, size, shape)]


@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: grad_key(*c))
def test_data_and_stride2_gradients_have_the_recorded_bits(case):
    got = grad_digest(*case)
    print("GRAD BITS %s: %s" % (grad_key(*case), got))
    assert got == _record(GRAD_RECORD)[grad_key(*case)]


def test_thin_tree_shapes_have_the_slices_they_were_chosen_for():
    for shape, (S, L) in THIN_TREE_SHAPES.items():
        assert T.conv_wgrad_thin_slices(*shape) == (S, L), shape
        assert S > 32 and (S - 1) * L < shape[0] * shape[3] * shape[4] <= S * L      # a second tree level; S slices of L cover K


@pytest.mark.parametrize("case", THIN_CASES, ids=lambda c: thin_key(*c))
def test_thin_gradients_have_the_recorded_bits(case):
    got = thin_digest(*case)
    print("THIN BITS %s: %s" % (thin_key(*case), got))
    assert got == _record(THIN_RECORD)[thin_key(*case)]


def test_full_walk_has_the_recorded_bits(tmp_path):
    got = walk_digest(tmp_path)
    print("THIN BITS %s: %s" % (THIN_WALK, got))
    assert got == _record(THIN_RECORD)[THIN_WALK]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_steps_and_updates_have_the_recorded_bits(tmp_path, precision):
    got = step_digest(precision, tmp_path)
    print("TRAIN BITS step/%s: %s" % (precision, got))
    assert got["update"]["image"] == got["adam"]["image"]             # the host twin of the masters changes no bit of the image
    assert got == _record()["step/" + precision]
