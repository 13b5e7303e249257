"""GPU tests of DarknetTrainer(wgrad_precision="f16s3"): the gradient walk with dW of every stride-1 BatchNorm conv (a size of
train.WGRAD_SPLIT_SIZES, Cin a multiple of 32) through rtod_conv_wgrad_split, everything else — the head convs, the stride-2 convs,
the data gradients unless grad_precision says otherwise, BatchNorm and the joins — on the exact entries.  mini_cfg at 64x64, B = 3,
scope backbone, on an eval fp32 plan and on an eval f16s3 plan, alone and together with grad_precision="f16s3", through the helpers of
tests/scope_grad_cases.py; one run under batch statistics through the float64 reference of tests/test_bn_train_gpu.py (cpu_grads_bn).

The gate is the project's 4 x the float32 floor (over_the_floor), unchanged: the CPU check of the format (tests/
test_wgrad_split_host.py) puts its own error at 0.14 - 0.80 of the float32 floor, so a walk through it must sit where the exact walk
sits.

Measured on an MI355X, largest rms ratio / max ratio over the 14 convs and the four combinations: 2.06 (conv 1, split data gradients) /
3.07 (conv 12, f16s3 plan: the exact walk's own figure there); under batch statistics 0.96 / 1.05."""
import numpy as np
import pytest
import torch

import test_bn_train_gpu as BN
from backbone_grad_cases import BACKBONE, MINI_S2, TRAINABLE
from scope_grad_cases import _forward, _frames, _model, _same, check_training_steps, cpu_graph_grads, over_the_floor, scope_trainer, step_batch, tenth_heads
from realtimeobjectdetection_amd import cfgs, train as T

pytestmark = pytest.mark.gpu
HEADS = [14, 22]
RES, B = 64, 3
COMBOS = [("fp32", "fp32"), ("fp32", "f16s3"), ("f16s3", "fp32"), ("f16s3", "f16s3")]       # (plan precision, grad_precision), wgrad_precision f16s3 in all


def _trainer(tmp_path, precision, name="m", **kw):
    m = _model(tmp_path, cfgs.mini_cfg(RES, RES), RES, precision, BACKBONE, name=name)
    t = T.DarknetTrainer(m, trainable="backbone", **kw)
    t.min_box_size = 4
    return m, t


def _batch():
    return _frames(B, RES, None), [torch.from_numpy(im) for im in step_batch()[1]]


def _split_convs(layers, want_layers):
    return [c for c in want_layers if layers[c].stride == 1 and layers[c].size in T.WGRAD_SPLIT_SIZES and T.conv_wgrad_split_takes(layers[c].cin, layers[c].size)]


@pytest.mark.parametrize("precision,grad_precision", COMBOS)
def test_backbone_gradients_through_split_weight_gradients_against_autograd(tmp_path, precision, grad_precision):
    """dW of all 14 trainable convs of mini_cfg with wgrad_precision="f16s3" against float64 torch autograd of the trainable sub-graph
    pinned to the DEVICE's masks, rms and max of (dW_dev - dW_64) / max |dW_64| at most 4 x the same figures of float32 autograd:
    test_backbone_gradients_against_autograd's gate, unchanged.  The walk is repeatable bit for bit; its loss and head gradients are
    the exact trainer's; dW of exactly the convs the walk sends to the split entry differ from the exact walk's bits (with exact data
    gradients: a weight gradient feeds nothing behind it), and with no size in WGRAD_SPLIT_SIZES the walk is the exact walk."""
    m, t = _trainer(tmp_path, precision, grad_precision=grad_precision, wgrad_precision="f16s3")
    xd, bnd = _batch()
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads = t.backbone_gradients(xd, bnd)
    want_layers = TRAINABLE["mini"]
    assert t.wgrad_precision == "f16s3" and t.grad_precision == grad_precision and m.active_precision == precision
    assert int(t.status.item()) == 0 and sorted(grads) == want_layers
    loss2, _, again = t.backbone_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(grads[k], again[k]) for k in grads)
    t.wgrad_precision = "fp32"                                        # the same trainer with the exact weight gradients
    loss_x, head_x, exact = t.backbone_gradients(xd, bnd)
    t.wgrad_precision = "f16s3"
    assert _same(loss, loss_x) and all(_same(head_grads[k][0], head_x[k][0]) and _same(head_grads[k][1], head_x[k][1]) for k in head_x)
    layers, readers, member, scales = t._graph("backbone")
    differ = [c for c in want_layers if not _same(grads[c], exact[c])]
    sent = _split_convs(layers, want_layers)
    print("WGRAD_SPLIT_SIZES %s: convs sent to the split entry %s, convs whose dW bits differ from the exact walk's %s" % (T.WGRAD_SPLIT_SIZES, sent, differ))
    assert differ == sent                                             # the data gradients are the same in both walks: only dW of the sent convs moves
    assert bool(sent) == bool(T.WGRAD_SPLIT_SIZES)
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in want_layers if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, pres = cpu_graph_grads(m, t, B, torch.float64, masks, dzs, scope="backbone")
    floor, _ = cpu_graph_grads(m, t, B, torch.float32, masks, dzs, scope="backbone")
    over = over_the_floor("mini %s plan, data gradients %s, split weight gradients" % (precision, grad_precision), m, layers, want_layers, precision, B, grads, want, floor, pres)
    assert not over, (precision, grad_precision, "(conv, rms ratio, max ratio) over 4 x the float32 floor", over)


def test_the_entry_runs_in_the_walk_whatever_the_tuple_says(tmp_path, monkeypatch):
    """With both sizes in the tuple (the walk's rule is otherwise untouched) every stride-1 conv of mini_cfg with Cin % 32 == 0 goes
    through the split entry and stays inside the unchanged gate: the routing is tested even if the measurement has emptied the tuple."""
    monkeypatch.setattr(T, "WGRAD_SPLIT_SIZES", (1, 3))
    m, t = _trainer(tmp_path, "fp32", wgrad_precision="f16s3")
    xd, bnd = _batch()
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads = t.backbone_gradients(xd, bnd)
    t.wgrad_precision = "fp32"
    _, _, exact = t.backbone_gradients(xd, bnd)
    layers, readers, member, scales = t._graph("backbone")
    want_layers = TRAINABLE["mini"]
    sent = _split_convs(layers, want_layers)
    assert sent and {layers[c].size for c in sent} == {1, 3} and [c for c in want_layers if not _same(grads[c], exact[c])] == sent
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in want_layers if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, pres = cpu_graph_grads(m, t, B, torch.float64, masks, dzs, scope="backbone")
    floor, _ = cpu_graph_grads(m, t, B, torch.float32, masks, dzs, scope="backbone")
    over = over_the_floor("mini fp32 plan, split weight gradients of both sizes", m, layers, want_layers, "fp32", B, grads, want, floor, pres)
    assert not over, ("(conv, rms ratio, max ratio) over 4 x the float32 floor", over)


def test_fp32_wgrad_precision_is_the_trainer_without_the_argument(tmp_path):
    xd, bnd = _batch()
    m0, t0 = scope_trainer(tmp_path, cfgs.mini_cfg(RES, RES), RES, "fp32", name="plain", trainable="backbone", options=BACKBONE)
    m1, t1 = _trainer(tmp_path, "fp32", name="arg", wgrad_precision="fp32")
    for model in (m0, m1):
        _forward(model, xd)
        tenth_heads(model)
    l0, h0, g0 = t0.backbone_gradients(xd, bnd)
    l1, h1, g1 = t1.backbone_gradients(xd, bnd)
    assert t0.wgrad_precision == "fp32" and _same(l0, l1) and sorted(g0) == sorted(g1) == TRAINABLE["mini"]
    assert all(_same(g0[k], g1[k]) for k in g0) and all(_same(h0[k][0], h1[k][0]) and _same(h0[k][1], h1[k][1]) for k in h0)


@pytest.mark.parametrize("precision", ["fp32", "f16s3"])
def test_training_steps_through_split_weight_gradients_lower_the_loss(tmp_path, precision):
    """feed_forward_through_model(trainable="backbone", wgrad_precision="f16s3"): an SGD step and two Adam steps, each the optimiser's
    documented update of the gradients backbone_gradients returned for the state before it (check_training_steps).  Then the descent
    on its own, as tests/test_grad_split_walk_gpu.py argues it: a fresh model with the heads at a tenth, plain SGD at lr = 1e-7, four
    losses, each below the one before."""
    xd, bnd = _batch()
    m, t = _trainer(tmp_path, precision, wgrad_precision="f16s3")
    losses = check_training_steps(m, t, xd, bnd, "backbone", sorted(TRAINABLE["mini"] + HEADS), TRAINABLE["mini"], MINI_S2)
    print("check_training_steps, losses before each step:", losses)
    m2, t2 = _trainer(tmp_path, precision, name="descent", wgrad_precision="f16s3")
    _forward(m2, xd)
    tenth_heads(m2)
    t2.optimizer = T.HeadOptimizer("sgd", lr=1e-7)
    falls = [float(t2.feed_forward_through_model(xd, bnd)) for _ in range(4)]
    print("SGD at lr 1e-7, losses before each step: %s" % (falls,))
    assert all(b < a for a, b in zip(falls, falls[1:])), falls


def test_batch_statistics_walk_through_split_weight_gradients(tmp_path):
    """.train(), keep_bn_inputs, fp32 plan, scope backbone: batchnorm_gradients with wgrad_precision="f16s3" (no frozen scale, dz out of
    rtod_bn_grad) against float64 autograd of the sub-graph with training=True BatchNorm (tests/test_bn_train_gpu.py's cpu_grads_bn), the
    4 x gate of that file unchanged; dgamma and dbeta, which no weight gradient feeds, keep the exact walk's bits."""
    m, t, scope, xd, bnd, _ = BN._trainer(tmp_path, "mini-backbone")
    t.wgrad_precision = "f16s3"
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads, bn_grads = t.batchnorm_gradients(xd, bnd)
    listed = [c for c, _ in m.trainable_layers()]
    assert sorted(grads) == sorted(bn_grads) == listed and int(t.status.item()) == 0
    t.wgrad_precision = "fp32"
    loss_x, _, exact, bn_x = t.batchnorm_gradients(xd, bnd)
    t.wgrad_precision = "f16s3"
    layers, readers, member, scales = t._graph(scope)
    assert all(s is None for s in scales.values())
    assert _same(loss, loss_x) and all(_same(bn_grads[k][0], bn_x[k][0]) and _same(bn_grads[k][1], bn_x[k][1]) for k in bn_x)
    assert [c for c in listed if not _same(grads[c], exact[c])] == _split_convs(layers, listed)
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in listed if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, _ = BN.cpu_grads_bn(m, t, torch.float64, scope, masks, dzs, t._net_input, {})
    floor, _ = BN.cpu_grads_bn(m, t, torch.float32, scope, masks, dzs, t._net_input, {})
    over = []
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    for c in listed:
        g, w, f = grads[c].cpu().numpy().astype(np.float64), want[c][0], floor[c][0]
        ref = np.abs(w).max()
        e_dev, e_32 = (g - w) / ref, (f - w) / ref
        q_rms, q_max = rms(e_dev) / rms(e_32), float(np.abs(e_dev).max() / np.abs(e_32).max())
        print("batch statistics conv %d dW: rms ratio %.2f  max ratio %.2f" % (c, q_rms, q_max))
        if not (q_rms <= 4 and q_max <= 4):
            over.append((c, round(q_rms, 2), round(q_max, 2)))
    assert not over, ("(conv, rms ratio, max ratio) over 4 x the float32 floor", over)
