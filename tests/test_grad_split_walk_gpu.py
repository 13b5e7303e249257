"""GPU tests of DarknetTrainer(grad_precision="f16s3"): the gradient walk with the data gradient of every stride-1 3x3 conv (Cin a
multiple of 32) on the split-f16 tiles (rtod_conv_dgrad_split), everything else — the 1x1 data gradients (measured slower through the
split entry: train.GRAD_SPLIT_SIZES), stride-2 data gradients, every weight gradient, the joins — on the exact entries.  mini_cfg at 64x64, B = 3, scope backbone, on an eval fp32 plan and on an eval f16s3
plan, through the helpers of tests/scope_grad_cases.py.

The gate is the project's 4 x the float32 floor (over_the_floor), unchanged: the CPU check of the format (tests/
test_dgrad_split_host.py) puts its own error at 0.06 - 0.26 of the float32 floor, so a walk through it must sit where the exact walk
sits."""
import numpy as np
import pytest
import torch

from backbone_grad_cases import BACKBONE, MINI_S2, TRAINABLE
from scope_grad_cases import _forward, _frames, _model, _same, check_training_steps, cpu_graph_grads, over_the_floor, scope_trainer, step_batch, tenth_heads
from realtimeobjectdetection_amd import cfgs, train as T

pytestmark = pytest.mark.gpu
HEADS = [14, 22]
RES, B = 64, 3


def _trainer(tmp_path, precision, name="m", **kw):
    m = _model(tmp_path, cfgs.mini_cfg(RES, RES), RES, precision, BACKBONE, name=name)
    t = T.DarknetTrainer(m, trainable="backbone", **kw)
    t.min_box_size = 4
    return m, t


def _batch():
    return _frames(B, RES, None), [torch.from_numpy(im) for im in step_batch()[1]]


@pytest.mark.parametrize("precision", ["fp32", "f16s3"])
def test_backbone_gradients_through_split_data_gradients_against_autograd(tmp_path, precision):
    """dW of all 14 trainable convs of mini_cfg with grad_precision="f16s3" against float64 torch autograd of the trainable sub-graph
    pinned to the DEVICE's masks, rms and max of (dW_dev - dW_64) / max |dW_64| at most 4 x the same figures of float32 autograd:
    test_backbone_gradients_against_autograd's gate, unchanged.  The walk is repeatable bit for bit, its loss and head gradients are
    the exact trainer's (they lie in front of every data gradient), and the split entry is really on the path: dW of the convs
    behind a split data gradient differ from the exact walk's bits.  The measured ratios are printed.

    Measured on an MI355X, largest rms ratio / max ratio over the 14 convs: fp32 plan 2.05 / 2.18 (conv 1), f16s3 plan 2.06 (conv 1) /
    2.92 (conv 12); the exact walk's own figures on the same plans are 1.39 / 2.12 and 1.86 / 3.07 (tests/test_backbone_grad_gpu.py)."""
    m, t = _trainer(tmp_path, precision, grad_precision="f16s3")
    xd, bnd = _batch()
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads = t.backbone_gradients(xd, bnd)
    want_layers = TRAINABLE["mini"]
    assert t.grad_precision == "f16s3" and m.active_precision == precision and int(t.status.item()) == 0 and sorted(grads) == want_layers
    loss2, _, again = t.backbone_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(grads[k], again[k]) for k in grads)
    t.grad_precision = "fp32"                                         # the same trainer on the exact entries
    loss_x, head_x, exact = t.backbone_gradients(xd, bnd)
    t.grad_precision = "f16s3"
    assert _same(loss, loss_x) and all(_same(head_grads[k][0], head_x[k][0]) and _same(head_grads[k][1], head_x[k][1]) for k in head_x)
    differ = [c for c in want_layers if not _same(grads[c], exact[c])]
    print("convs whose dW bits differ from the exact walk's:", differ)
    assert differ and T.GRAD_SPLIT_SIZES == (3,)                      # (the 1x1 data gradients, the head convs' among them, stay exact: conv 21 keeps its bits)
    layers, readers, member, scales = t._graph("backbone")
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in want_layers if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, pres = cpu_graph_grads(m, t, B, torch.float64, masks, dzs, scope="backbone")
    floor, _ = cpu_graph_grads(m, t, B, torch.float32, masks, dzs, scope="backbone")
    over = over_the_floor("mini %s, split data gradients" % precision, m, layers, want_layers, precision, B, grads, want, floor, pres)
    assert not over, (precision, "(conv, rms ratio, max ratio) over 4 x the float32 floor", over)


def test_fp32_grad_precision_is_the_trainer_without_the_argument(tmp_path):
    xd, bnd = _batch()
    m0, t0 = scope_trainer(tmp_path, cfgs.mini_cfg(RES, RES), RES, "fp32", name="plain", trainable="backbone", options=BACKBONE)
    m1, t1 = _trainer(tmp_path, "fp32", name="arg", grad_precision="fp32")
    for model in (m0, m1):
        _forward(model, xd)
        tenth_heads(model)
    l0, h0, g0 = t0.backbone_gradients(xd, bnd)
    l1, h1, g1 = t1.backbone_gradients(xd, bnd)
    assert t0.grad_precision == "fp32" and _same(l0, l1) and sorted(g0) == sorted(g1) == TRAINABLE["mini"]
    assert all(_same(g0[k], g1[k]) for k in g0) and all(_same(h0[k][0], h1[k][0]) and _same(h0[k][1], h1[k][1]) for k in h0)


@pytest.mark.parametrize("precision", ["fp32", "f16s3"])
def test_training_steps_through_split_data_gradients_lower_the_loss(tmp_path, precision):
    """feed_forward_through_model(trainable="backbone", grad_precision="f16s3"): an SGD step and two Adam steps, each the optimiser's
    documented update of the gradients backbone_gradients returned for the state before it (check_training_steps).

    Then the loss falls.  check_training_steps fixes lr = 1e-4, which is a statement about the optimiser's arithmetic, not a step
    size for these synthetic weights: on the full-strength synthetic heads the SGD step at 1e-4 overshoots whatever computes the
    gradient (measured on an MI355X, fp32 plan: 709.8 -> 7059.6 -> 1065.4).  So the descent is checked on its own: a fresh model with
    the heads at a tenth (sigmoids that do not saturate, as in the gradient tests), plain SGD at lr = 1e-7 — inside the range in which
    the directional-derivative tests find the loss linear along -g, and with ||g||^2 of order 1e6 a first-order decrease of order
    0.1 per step, far above the float32 noise of the loss — four losses, each below the one before."""
    xd, bnd = _batch()
    m, t = _trainer(tmp_path, precision, grad_precision="f16s3")
    losses = check_training_steps(m, t, xd, bnd, "backbone", sorted(TRAINABLE["mini"] + HEADS), TRAINABLE["mini"], MINI_S2)
    print("check_training_steps, losses before each step:", losses)
    m2, t2 = _trainer(tmp_path, precision, name="descent", grad_precision="f16s3")
    _forward(m2, xd)
    tenth_heads(m2)
    t2.optimizer = T.HeadOptimizer("sgd", lr=1e-7)
    _, _, g = t2.backbone_gradients(xd, bnd)
    g2 = sum(float((dw.double() ** 2).sum()) for dw in g.values())
    falls = [float(t2.feed_forward_through_model(xd, bnd)) for _ in range(4)]
    print("SGD at lr 1e-7, ||g||^2 of the trained convs %.6g, losses before each step: %s" % (g2, falls))
    assert all(b < a for a, b in zip(falls, falls[1:])), falls
