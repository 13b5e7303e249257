"""GPU tests of the neck training path: rtod_conv_dgrad (csrc/dgrad.hip) and rtod_upsample2x_grad (csrc/upsample_grad.hip) against exact
integer and float64 results, option keep_neck_activations, and DarknetTrainer.neck_gradients / feed_forward_through_model(trainable=
"neck") end to end against torch autograd of the neck sub-graph.

Gates, with u = 2^-24.
* Integers: operands in [-4, 4], power-of-two scales and the slope 0.5 make every product and partial sum exactly representable
  (16 * 9 * Cout < 2^24), so the results equal the int64 sums bit for bit in any order.
* dgrad on floats: |dx - float64| <= ((K + 2) u + 2^-52) |m| sum |w s| |dz|, K = size^2 * Cout: one rounding of the folded weight v
  (the double product's own 2^-53 is the 2^-52 term with the float rounding's cross term), a K-term fmaf chain, the mask
  multiplication.  A size-3 call keeps one chain per tap and adds the nine tap sums: Cout + 8 roundings on the way of a term
  instead of 9 Cout, inside the same bound.  The second-order terms of the worst case — (K u)^2 / (1 - K u) of the chain, 2 K u^2
  of the cross terms, at most 2e-8 of the mass at K = 2295 against the gate's 1.4e-4 — are left out as in
  tests/test_block_grad_gpu.py: a K-term chain of random signs errs by about sqrt(K) u, far inside.
* upsample grad: integer dz make every bilinear sum an exact multiple of 1/16: float64 autograd of F.interpolate bit for bit.
* End to end: the docstrings of the tests."""
import functools

import numpy as np
import pytest
import torch

from neck_grad_cases import DGRAD_SHAPES, NECK, U, UPSAMPLE_SHAPES, conv_dgrad_ref
from scope_grad_cases import KEEP, _dev, _forward, _frames, _model, _same, check_directional_derivative, check_training_steps, cpu_graph_grads, cpu_scope_loss
from scope_grad_cases import over_the_floor, scope_trainer, step_batch, tenth_heads
from realtimeobjectdetection_amd import cfgs, train as T

pytestmark = pytest.mark.gpu
F = np.float32
KEEP = KEEP["neck"]
fn = torch.nn.functional


# ------------------------------------------------------------------------------------------ 4 / 5. the data gradient
def _dgrad(w, dz, size, scale=None, y=None, slope=1.0):
    return T.conv_dgrad_async(_dev(w), _dev(dz), size, None if scale is None else _dev(scale), None if y is None else _dev(y), slope).cpu().numpy()


@pytest.mark.parametrize("size", [3, 1])
@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_conv_dgrad_exact_on_small_integers(shape, size):
    B, cout, cin, H, W = shape
    assert 16 * 9 * cout < 2 ** 24
    rng = np.random.default_rng(B * 1000 + H * W + size)
    w, dz, y = rng.integers(-4, 5, (cout, cin, size, size)), rng.integers(-4, 5, (B, cout, H, W)), rng.integers(-1, 2, (B, cin, H, W))
    want = conv_dgrad_ref(w, dz, np.int64).astype(np.float64)
    wf, dzf, yf = w.astype(F), dz.astype(F), y.astype(F)
    m = np.where(y > 0, 1.0, 0.5)                                     # y == 0 takes the slope
    assert np.array_equal(_dgrad(wf, dzf, size, None, yf, 0.5).astype(np.float64), want * m), (shape, size)
    assert np.array_equal(_dgrad(wf, dzf, size, None, None, 0.5).astype(np.float64), want), (shape, size)        # no y: linear
    assert np.array_equal(_dgrad(wf, dzf, size, None, yf, 1.0).astype(np.float64), want), (shape, size)          # slope 1: linear
    if H == 1 and W == 1:                                             # only the centre tap sees the pixel
        assert np.array_equal(want[:, :, 0, 0], np.einsum("oc,bo->bc", w[:, :, size // 2, size // 2], dz[:, :, 0, 0])) and want.any()
    s = 2.0 ** rng.integers(-3, 4, cout).astype(np.float64)           # power-of-two row scales keep the integers exact
    wants = conv_dgrad_ref(w.astype(np.float64) * s[:, None, None, None], dz, np.float64)
    assert np.array_equal(_dgrad(wf, dzf, size, s, yf, 0.5).astype(np.float64), wants * m), (shape, size)


@pytest.mark.parametrize("size", [3, 1])
@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_conv_dgrad_floats_within_the_chain_bound_and_reproducible(shape, size):
    B, cout, cin, H, W = shape
    K = size * size * cout
    rng = np.random.default_rng(B * 77 + H * W + size)
    w, dz, y = (rng.standard_normal(s).astype(F) for s in ((cout, cin, size, size), (B, cout, H, W), (B, cin, H, W)))
    y[0, 0, 0, 0] = 0.0
    s = (rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float64)
    slope = F(0.1)
    m = np.where(y > 0, 1.0, float(slope))
    for scale in (None, s):
        v64 = w.astype(np.float64) * (1.0 if scale is None else scale[:, None, None, None])
        dx = _dgrad(w, dz, size, scale, y, float(slope))
        want = m * conv_dgrad_ref(v64, dz, np.float64)
        bound = ((K + 2) * U + 2.0 ** -52) * m * conv_dgrad_ref(np.abs(v64), np.abs(dz), np.float64)
        worst = float(np.divide(np.abs(dx - want), bound, out=np.zeros_like(want), where=bound > 0).max())
        print("dgrad %s size %d %s: worst error / bound %.3g" % (shape, size, "scaled" if scale is not None else "plain", worst))
        assert (np.abs(dx - want) <= bound).all(), (shape, size, scale is not None, worst)
        assert dx.tobytes() == _dgrad(w, dz, size, scale, y, float(slope)).tobytes(), (shape, size)
    if size == 1:                                                     # the 1x1 instance without a scale is rtod_conv1x1_dgrad, bit for bit
        old = T.conv1x1_dgrad_async(_dev(w), _dev(dz), _dev(y), float(slope)).cpu().numpy()
        assert old.tobytes() == _dgrad(w, dz, 1, None, y, float(slope)).tobytes(), shape


# ------------------------------------------------------------------------------------------ 6. the upsample backward
@pytest.mark.parametrize("channels", [3, 33])
@pytest.mark.parametrize("hw", UPSAMPLE_SHAPES)
def test_upsample2x_grad_is_float64_autograd_bit_for_bit(hw, channels):
    (H, W), B = hw, 2
    rng = np.random.default_rng(H * 100 + W + channels)
    dz, y = rng.integers(-4, 5, (B, channels, 2 * H, 2 * W)).astype(F), rng.integers(-1, 2, (B, channels, H, W)).astype(F)
    for mode in ("bilinear", "nearest"):
        x = torch.zeros((B, channels, H, W), dtype=torch.float64, requires_grad=True)
        up = fn.interpolate(x, scale_factor=2, mode=mode, align_corners=False) if mode == "bilinear" else fn.interpolate(x, scale_factor=2, mode=mode)
        up.backward(torch.from_numpy(dz.astype(np.float64)))
        want = x.grad.numpy()
        assert np.array_equal(want * 16, np.rint(want * 16)) and np.abs(want).max() > 0
        got = T.upsample2x_grad_async(_dev(dz), None, 1.0, mode).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (hw, channels, mode)
        fused = T.upsample2x_grad_async(_dev(dz), _dev(y), 0.5, mode).cpu().numpy()
        assert np.array_equal(fused.astype(np.float64), want * np.where(y > 0, 1.0, 0.5)), (hw, channels, mode)
        assert np.array_equal(T.upsample2x_grad_async(_dev(dz), _dev(y), 1.0, mode).cpu().numpy(), got)
        assert fused.tobytes() == T.upsample2x_grad_async(_dev(dz), _dev(y), 0.5, mode).cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------ 7. keep_neck_activations alone
@pytest.mark.parametrize("net,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "f16", None), ("mini", "fp32", 96), ("tiny", "fp32", None)])
def test_keep_neck_activations_changes_no_output_bit(tmp_path, net, precision, width):
    res, B = 64, 3
    text = cfgs.mini_cfg(res, width or res) if net == "mini" else cfgs.yolov3_tiny_cfg(res, res)
    x = _frames(B, res, width)
    off = _model(tmp_path, text, res, precision, name="off")
    on = _model(tmp_path, text, res, precision, {"keep_neck_activations": 1}, name="on")
    every = _model(tmp_path, text, res, precision, keep_all=True, name="all")
    for model in (off, on, every):
        model.input_width = width
    for td in (False, True):
        y_off, y_on, y_all = _forward(off, x, td), _forward(on, x, td), _forward(every, x, td)
        assert _same(y_off, y_on) and _same(y_off, y_all)
        assert [c for c, _ in on.neck_layers()] == NECK[net]
        for conv, inp in on.neck_layers():                            # what the walk reads is what a plan that keeps everything holds
            for layer in (conv, inp):
                got, want = on.read_layer(layer, B), every.read_layer(layer, B)
                assert got.abs().sum() > 0 and torch.equal(got, want), (net, precision, layer)
    assert [li.variant for li in off.launch_infos()] == [li.variant for li in on.launch_infos()]
    assert on._info.arena_bytes >= off._info.arena_bytes


# ------------------------------------------------------------------------------------------ 8. neck_gradients against autograd
_neck_trainer = functools.partial(scope_trainer, trainable="neck", options=KEEP)
_cpu_neck_grads = functools.partial(cpu_graph_grads, scope="neck")   # autograd of the neck sub-graph (scope_grad_cases.cpu_graph) with the DEVICE's masks


@pytest.mark.parametrize("net,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "fp32", 96), ("tiny", "fp32", None)])
def test_neck_gradients_against_autograd(tmp_path, net, precision, width):
    """dW of DarknetTrainer.neck_gradients for every neck conv against torch autograd of the neck sub-graph (scope_grad_cases.cpu_graph) with the DEVICE's
    masks, fed the device's boundary inputs and pulled back from the device's dz, once in float64 (the truth) and once in float32
    torch (the reference's own arithmetic, the floor).

    The masks.  As in test_block_gradients_against_autograd, unchanged: a flip of the device's mask against the float64 forward's
    pre-activation is legitimate only where |pre_64| is within the forward's own error, (K1 + 2) u (sum |w s| |x| + |bias|) at fp32
    and 1e-4 (f16s3) of that mass.

    The gate per neck conv: rms and max of (dW_dev - dW_64) / max |dW_64| are at most 4 x the same figures of (dW_32 - dW_64), the
    project's 4 x the float32 floor, measured against the reference arithmetic.

    Measured on an MI355X, rms ratio / max ratio per conv (no mask flipped anywhere):
      mini 64 fp32     12: 1.63 / 2.08   13: 1.01 / 1.09   17: 1.21 / 1.16   20: 1.38 / 1.74   21: 0.92 / 1.03
      mini 64 f16s3    12: 1.51 / 1.90   13: 1.16 / 1.63   17: 1.23 / 1.64   20: 1.28 / 1.35   21: 0.96 / 0.97
      mini 64x96 fp32  12: 1.67 / 1.42   13: 1.03 / 0.91   17: 1.21 / 0.94   20: 1.25 / 1.31   21: 0.77 / 0.58
      tiny 64 fp32     12: 1.19 / 0.93   13: 1.44 / 1.37   14: 1.10 / 1.05   18: 1.11 / 1.09   21: 0.91 / 0.76
    With ONE fmaf chain over all 9 * Cout terms of a 3x3 data gradient, conv 12 (behind conv 13's K = 9216) and conv 20 (behind conv
    21's K = 4608) stood at 4.19 - 4.41 x in the maximum and this test failed in its three mini cases; the kernel now keeps one chain
    per tap and adds the nine tap sums in order (csrc/dgrad.hip)."""
    res, B = 64, 3
    text = cfgs.mini_cfg(res, width or res) if net == "mini" else cfgs.yolov3_tiny_cfg(res, res)
    m, t = _neck_trainer(tmp_path, text, res, precision, width)
    xd = _frames(B, res, width)
    bnd = [torch.from_numpy(im) for im in step_batch()[1]]
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, neck_grads = t.neck_gradients(xd, bnd)
    assert m.active_precision == precision and int(t.status.item()) == 0 and sorted(neck_grads) == NECK[net] == [c for c, _ in m.neck_layers()]
    # twice the same bytes; the heads' part is head_gradients; the block convs' entries are block_gradients of a "blocks" trainer
    loss2, _, again = t.neck_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(neck_grads[k], again[k]) for k in neck_grads)
    loss_h, grads_h = t.head_gradients(xd, bnd)
    assert _same(loss, loss_h) and all(_same(head_grads[k][0], grads_h[k][0]) and _same(head_grads[k][1], grads_h[k][1]) for k in grads_h)
    mb, tb = _neck_trainer(tmp_path, text, res, precision, width, name="blocks", trainable="blocks", options={"keep_head_inputs": 1, "keep_block_inputs": 1})
    _forward(mb, xd)
    tenth_heads(mb)
    loss_b, _, block_grads = tb.block_gradients(xd, bnd)
    assert _same(loss, loss_b) and len(block_grads) == len(m.head_layers()) and all(_same(neck_grads[k], block_grads[k]) for k in block_grads)
    # the CPU model with the device's masks
    layers, readers, member, scales = t._graph("neck")
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in NECK[net] if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, pres = _cpu_neck_grads(m, t, B, torch.float64, masks, dzs)
    floor, _ = _cpu_neck_grads(m, t, B, torch.float32, masks, dzs)
    over = over_the_floor("%s %s" % (net, precision), m, layers, NECK[net], precision, B, neck_grads, want, floor, pres)
    if net == "mini" and width is None:                               # the fan-out sum: layer 12 is read by conv 13 and by route 16
        assert readers[12] == [13, 16] and neck_grads[12].abs().sum() > 0
        for cut in ((12, 13), (12, 16)):
            part, _ = _cpu_neck_grads(m, t, B, torch.float64, masks, dzs, cut=cut)
            assert not np.allclose(part[12], want[12], rtol=1e-3, atol=1e-6 * np.abs(want[12]).max()) and np.abs(part[12]).max() > 0, cut
            assert all(np.array_equal(part[c], want[c]) for c in (13, 17, 20, 21))
    assert not over, (net, precision, "(conv, rms ratio, max ratio) over 4 x the float32 floor", over)      # after every figure is printed


# ------------------------------------------------------------------------------------------ 9. the directional derivative
def test_the_loss_falls_along_the_neck_gradient_by_what_it_says(tmp_path):
    """The central difference of the device loss along -g, all five neck convs of mini_cfg(64, 64) moved together by update_conv_weight,
    against ||g||^2 of neck_gradients (fp32 plan, the batch of step_batch), in the manner of
    test_the_loss_falls_along_the_block_gradient_by_what_it_says: eps and the allowed gap come from the float64 CPU model of the neck on
    the device's boundary inputs with torch's own leaky_relu, never from a device result — eps is the smallest of 1e-2, 3e-3, ... at
    which the modelled truncation gap still exceeds the float32 evaluation noise tenfold, and the test allows
    4 * |fd_cpu - dd_cpu| + 2 * noise / (2 eps), dd_cpu the model's central difference at a tenth of eps."""
    B = 3
    m, t = _neck_trainer(tmp_path, cfgs.mini_cfg(64, 64), 64, "fp32")
    x, images = step_batch()
    xd, bnd = torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images]
    _, _, grads = t.neck_gradients(xd, bnd)
    l0 = float(t.last_components[0].item())
    assert sorted(grads) == NECK["mini"]
    check_directional_derivative(m, t, xd, bnd, grads, cpu_scope_loss(m, t, B, images, grads, "neck"), l0)


# ------------------------------------------------------------------------------------------ 10. the training step
@pytest.mark.parametrize("precision,width", [("fp32", None), ("f16s3", None), ("f16s3", 96)])
def test_training_step_on_the_neck(tmp_path, precision, width):
    """feed_forward_through_model(trainable="neck"), an SGD step and then two Adam steps: after each, the masters and moments of the
    heads and of all five neck convs equal block_grad_cases.opt_update_f32 of the gradients neck_gradients returned for the state
    before the step (every gradient kernel is enqueued before the first step), and the packed image, as uint32 words, equals the host
    pack of the synchronised parameters.  The loss of the next forward differs from the first.  A trainable="blocks" trainer computes
    the same bits on a plan with and without the new option."""
    text = cfgs.mini_cfg(64, width or 64)
    xd, bnd = _frames(3, 64, width), [torch.from_numpy(im) for im in step_batch()[1]]
    m, t = _neck_trainer(tmp_path, text, 64, precision, width)
    layers = [12, 13, 14, 17, 20, 21, 22]
    losses = check_training_steps(m, t, xd, bnd, "neck", layers, NECK["mini"], [12])
    # the block path on a twin: the same bits with and without the new option
    out = []
    for name, options in (("b0", {"keep_head_inputs": 1, "keep_block_inputs": 1}), ("b1", dict(KEEP, keep_block_inputs=1))):
        mb, tb = _neck_trainer(tmp_path, text, 64, precision, width, name=name, trainable="blocks", options=options)
        tb.optimizer.lr = 1e-4
        out.append(([tb.feed_forward_through_model(xd, bnd) for _ in range(2)], mb.packed_weights(), sorted(tb.optimizer.state)))
    assert all(_same(a, b) for a, b in zip(out[0][0], out[1][0])) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] == [13, 14, 21, 22]
    assert float(out[0][0][0]) == losses[0]
