"""GPU tests of the "full" training path: rtod_maxpool_grad (csrc/maxpool_grad.hip), rtod_conv_wgrad_thin (csrc/wgrad.hip) and
rtod_conv_dgrad_thin (csrc/dgrad.hip) against exact integer and float64 results, and DarknetTrainer.full_gradients /
feed_forward_through_model(trainable="full") end to end against torch autograd of the full sub-graph of pool_train_mini_cfg and on
YOLOv3-tiny itself.

Gates, with u = 2^-24.
* max-pool backward on {0, 1, 2}: ties everywhere, every sum exact: bit-equal to float32 CPU autograd of nn.MaxPool2d(2, 2) /
  replicate pad + nn.MaxPool2d(2, 1), and with slope 0.1 to that times torch's mask expression.  On floats with slope 1: an element is
  0 + c1 (exact) and at most three more fp32 adds: |dx - float64| <= 3 u sum |contributions|.
* thin wgrad on floats: |dW - float64| <= (L + S + 2) u sum |dz x| with L, S from rtod_conv_wgrad_thin_slices: an L-term fmaf chain,
  at most S adds of the reduction (the two-level tree has fewer on every path), the row scale's rounding, and the double product's
  2^-53 under the same 2^-52 as the dgrad gate.  Second-order terms are left out as in tests/test_block_grad_gpu.py.
* thin dgrad on floats: the per-tap chain bound of tests/test_neck_grad_gpu.py, K = size^2 Cout.
* End to end: the docstrings of the tests."""
import numpy as np
import pytest
import torch

from block_grad_cases import wgrad_ref
from full_grad_cases import (DGRAD_THIN_SHAPES, FULL, POOL_MINI_FULL, POOL_SHAPES, TINY_FULL, U, WGRAD_THIN_SHAPES, full_batch, maxpool_grad_ref,
                             pool_out_hw, pool_winners, torch_pool_grad, winner_flips_within_the_forward_error)
from neck_grad_cases import conv_dgrad_ref
from scope_grad_cases import _dev, _forward, _frames, _same, check_directional_derivative, check_training_steps, cpu_graph_grads, cpu_scope_loss
from scope_grad_cases import over_the_floor, scope_trainer, tenth_heads
from realtimeobjectdetection_amd import cfgs, synth, train as T

pytestmark = pytest.mark.gpu
F = np.float32
fn = torch.nn.functional


# ------------------------------------------------------------------------------------------ 1. the max-pool backward
def _pool(dz, x, slope, stride):
    return T.maxpool_grad_async(_dev(dz), _dev(x), slope, 2, stride).cpu().numpy()


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_grad_is_autograd_bit_for_bit_on_ties(shape):
    B, C_, H, W, stride = shape
    Ho, Wo = pool_out_hw(H, W, stride)
    rng = np.random.default_rng(B * 1000 + H * W + stride)
    x, dz = rng.integers(0, 3, (B, C_, H, W)).astype(F), rng.integers(0, 3, (B, C_, Ho, Wo)).astype(F)
    want = torch_pool_grad(dz, x, stride)                             # float32 CPU autograd of the reference's module
    got = _pool(dz, x, 1.0, stride)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), shape
    xt = torch.from_numpy(x)
    masked = (torch.from_numpy(want) * torch.full_like(xt, 0.1).masked_fill_(xt > 0, 1)).numpy()
    assert _pool(dz, x, 0.1, stride).tobytes() == masked.tobytes(), shape
    if stride == 2:                                                   # an odd last row / column is covered by no window: exact +0
        assert not got[:, :, 2 * Ho:, :].tobytes().strip(b"\0") and not got[:, :, :, 2 * Wo:].tobytes().strip(b"\0")


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_grad_floats_within_three_roundings_and_reproducible(shape):
    B, C_, H, W, stride = shape
    Ho, Wo = pool_out_hw(H, W, stride)
    rng = np.random.default_rng(B * 77 + H * W + stride)
    x, dz = rng.standard_normal((B, C_, H, W)).astype(F), rng.standard_normal((B, C_, Ho, Wo)).astype(F)
    want, mass = maxpool_grad_ref(dz, x, stride, np.float64)
    got = _pool(dz, x, 1.0, stride)
    worst = float(np.divide(np.abs(got - want), 3 * U * mass, out=np.zeros_like(want), where=mass > 0).max())
    print("maxpool_grad %s: worst error / bound %.3g" % (shape, worst))
    assert (np.abs(got - want) <= 3 * U * mass).all(), (shape, worst)
    assert got.tobytes() == _pool(dz, x, 1.0, stride).tobytes()
    m = np.where(x > 0, F(1.0), F(0.1)).astype(F)
    assert _pool(dz, x, 0.1, stride).tobytes() == (got * m).astype(F).tobytes()          # one more fp32 multiplication


# ------------------------------------------------------------------------------------------ 2. the thin weight gradient
def _wgrad(dz, x, size, scale=None):
    return T.conv_wgrad_thin_async(_dev(dz), _dev(x), size, None if scale is None else _dev(scale)).cpu().numpy()


@pytest.mark.parametrize("shape", WGRAD_THIN_SHAPES)
def test_conv_wgrad_thin_exact_on_small_integers(shape):
    B, cout, cin, H, W, size = shape
    assert 4 * B * H * W < 2 ** 24
    rng = np.random.default_rng(B * 1000 + H * W + size + cin)
    dz, x = rng.integers(-2, 3, (B, cout, H, W)), rng.integers(-2, 3, (B, cin, H, W))
    want = wgrad_ref(dz, x, size, np.int64).astype(np.float64)
    got = _wgrad(dz.astype(F), x.astype(F), size)
    assert got.shape == (cout, cin, size, size) and np.array_equal(got.astype(np.float64), want), shape
    s = 2.0 ** rng.integers(-3, 4, cout).astype(np.float64)           # the row scale, applied once: powers of two keep the integers exact
    assert np.array_equal(_wgrad(dz.astype(F), x.astype(F), size, s).astype(np.float64), want * s[:, None, None, None]), shape
    routed = T.conv_wgrad_async(_dev(dz.astype(F)), _dev(x.astype(F)), size)       # Cin % 32 != 0: conv_wgrad_async takes the thin entry
    assert routed[1] is None and np.array_equal(routed[0].cpu().numpy(), got)


@pytest.mark.parametrize("shape", WGRAD_THIN_SHAPES)
def test_conv_wgrad_thin_floats_within_the_summation_bound_and_reproducible(shape):
    B, cout, cin, H, W, size = shape
    S, L = T.conv_wgrad_thin_slices(B, cout, cin, H, W, size)
    if shape == WGRAD_THIN_SHAPES[-1]:
        assert S >= 3 and (B * H * W) % L != 0
    rng = np.random.default_rng(B * 77 + H * W + size + cin)
    dz, x = rng.standard_normal((B, cout, H, W)).astype(F), rng.standard_normal((B, cin, H, W)).astype(F)
    s = (rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float64)
    mass = wgrad_ref(np.abs(dz), np.abs(x), size, np.float64)
    for scale in (None, s):
        k = 1.0 if scale is None else scale[:, None, None, None]
        want = wgrad_ref(dz, x, size, np.float64) * k
        bound = ((L + S + 2) * U + 2.0 ** -52) * mass * np.abs(k)
        got = _wgrad(dz, x, size, scale)
        worst = float(np.divide(np.abs(got - want), bound, out=np.zeros_like(want), where=bound > 0).max())
        print("wgrad_thin %s (S %d, L %d) %s: worst error / bound %.3g" % (shape, S, L, "scaled" if scale is not None else "plain", worst))
        assert (np.abs(got - want) <= bound).all(), (shape, scale is not None, worst)
        assert got.tobytes() == _wgrad(dz, x, size, scale).tobytes(), shape


# ------------------------------------------------------------------------------------------ 3. the thin data gradient
def _dgrad(w, dz, size, scale=None, y=None, slope=1.0):
    return T.conv_dgrad_thin_async(_dev(w), _dev(dz), size, None if scale is None else _dev(scale), None if y is None else _dev(y), slope).cpu().numpy()


@pytest.mark.parametrize("shape", DGRAD_THIN_SHAPES)
def test_conv_dgrad_thin_exact_on_small_integers(shape):
    B, cout, cin, H, W, size = shape
    assert 16 * 9 * cout < 2 ** 24
    rng = np.random.default_rng(B * 1000 + H * W + size + cin)
    w, dz, y = rng.integers(-4, 5, (cout, cin, size, size)), rng.integers(-4, 5, (B, cout, H, W)), rng.integers(-1, 2, (B, cin, H, W))
    want = conv_dgrad_ref(w, dz, np.int64).astype(np.float64)
    wf, dzf, yf = w.astype(F), dz.astype(F), y.astype(F)
    m = np.where(y > 0, 1.0, 0.5)
    got = _dgrad(wf, dzf, size, None, yf, 0.5)
    assert got.shape == (B, cin, H, W) and np.array_equal(got.astype(np.float64), want * m), shape
    assert np.array_equal(_dgrad(wf, dzf, size, None, None, 0.5).astype(np.float64), want), shape
    assert np.array_equal(_dgrad(wf, dzf, size, None, yf, 1.0).astype(np.float64), want), shape
    s = 2.0 ** rng.integers(-3, 4, cout).astype(np.float64)
    wants = conv_dgrad_ref(w.astype(np.float64) * s[:, None, None, None], dz, np.float64)
    assert np.array_equal(_dgrad(wf, dzf, size, s, yf, 0.5).astype(np.float64), wants * m), shape
    routed = T.conv_dgrad_async(_dev(wf), _dev(dzf), size, None, _dev(yf), 0.5).cpu().numpy()      # Cin % 32 != 0: the thin entry
    assert np.array_equal(routed, got)


@pytest.mark.parametrize("shape", DGRAD_THIN_SHAPES)
def test_conv_dgrad_thin_floats_within_the_chain_bound_and_reproducible(shape):
    B, cout, cin, H, W, size = shape
    K = size * size * cout
    rng = np.random.default_rng(B * 77 + H * W + size + cin)
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
        print("dgrad_thin %s %s: worst error / bound %.3g" % (shape, "scaled" if scale is not None else "plain", worst))
        assert (np.abs(dx - want) <= bound).all(), (shape, scale is not None, worst)
        assert dx.tobytes() == _dgrad(w, dz, size, scale, y, float(slope)).tobytes(), shape


# ------------------------------------------------------------------------------------------ 4. full_gradients against autograd
def _full_trainer(tmp_path, height, width, precision, stem, name="m", trainable="full", options=None, classes=3):
    text = cfgs.pool_train_mini_cfg(height, width, classes=classes, stem=stem)
    return scope_trainer(tmp_path, text, height, precision, None if width == height else width, name=name, trainable=trainable, options=FULL if options is None else options)


def _batch(height, width, classes=3, B=3):
    xd = _frames(B, height, None if width == height else width)
    return xd, [torch.from_numpy(im) for im in full_batch(height, width, classes, B)]


@pytest.mark.parametrize("height,width,precision,stem", [(64, 64, "fp32", 16), (64, 96, "fp32", 16), (40, 40, "fp32", 16), (64, 64, "f16s3", 32)])
def test_full_gradients_against_autograd(tmp_path, height, width, precision, stem):
    """dW of DarknetTrainer.full_gradients for every conv of the full graph of pool_train_mini_cfg against torch autograd of that
    sub-graph (scope_grad_cases.cpu_graph) with the DEVICE's leaky masks and the DEVICE's pool winners, fed the prepared network
    input (or, where layer 0 is no member, the device's boundary inputs) and pulled back from the device's dz, once in float64 (the
    truth) and once in float32 torch (the floor).

    The masks: scope_grad_cases.over_the_floor's rule, unchanged.  The winners: where the device's winner of a window is not the maximum
    of the float64 model's values, the two values may differ by no more than the forward's own error of the conv that produced them,
    (K + 2) u x mass at fp32 and 1e-4 x mass at f16s3, the winner's and the maximum's masses added; any other flip fails.

    The gate per conv: rms and max of (dW_dev - dW_64) / max |dW_64| are at most 4 x the same figures of (dW_32 - dW_64).

    Measured on an MI355X, rms ratio / max ratio per conv (no mask and no winner flipped anywhere):
      64x64 fp32 stem 16   0: 1.02 / 1.01  2: 1.32 / 1.55  4: 0.92 / 0.76  6: 0.97 / 0.75  8: 0.76 / 0.66  9: 1.10 / 1.26  10: 0.80 / 0.81  14: 0.97 / 1.42  17: 0.33 / 0.19
      64x96 fp32 stem 16   0: 1.34 / 1.09  2: 1.40 / 2.02  4: 0.63 / 0.35  6: 0.85 / 0.58  8: 0.65 / 0.36  9: 1.04 / 1.60  10: 0.75 / 0.57  14: 0.85 / 0.76  17: 0.24 / 0.21
      40x40 fp32 stem 16   0: 0.84 / 0.93  2: 0.86 / 0.80  4: 0.82 / 0.96  6: 0.95 / 0.87  8: 0.90 / 0.78  9: 1.00 / 1.27  10: 0.89 / 0.62  14: 0.91 / 0.63  17: 0.56 / 0.39
      64x64 f16s3 stem 32                  2: 1.26 / 1.18  4: 0.81 / 0.65  6: 0.96 / 0.94  8: 0.75 / 0.59  9: 1.10 / 0.87  10: 0.96 / 0.69  14: 0.92 / 0.56  17: 0.36 / 0.22"""
    B = 3
    m, t = _full_trainer(tmp_path, height, width, precision, stem)
    xd, bnd = _batch(height, width)
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads = t.full_gradients(xd, bnd)
    convs = POOL_MINI_FULL[stem]
    assert m.active_precision == precision and int(t.status.item()) == 0 and sorted(grads) == convs == [c for c, _ in m.full_layers()]
    loss2, _, again = t.full_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(grads[k], again[k]) for k in grads)
    layers, readers, member, scales = t._graph("full")
    pools = [L.index for L in layers if L.type == "maxpool" and member[L.index]]
    assert len(pools) == 4
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in convs if layers[c].leaky}
    winners = {p: pool_winners(m.read_layer(p - 1, B).cpu().numpy(), layers[p].stride) for p in pools}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    x_in = t._net_input
    want, pres = cpu_graph_grads(m, t, B, torch.float64, masks, dzs, scope="full", x_in=x_in, winners=winners)
    floor, _ = cpu_graph_grads(m, t, B, torch.float32, masks, dzs, scope="full", x_in=x_in, winners=winners)
    label = "pool_mini %dx%d %s stem %d" % (height, width, precision, stem)
    for p in pools:
        n = winner_flips_within_the_forward_error(label, m, layers, p, winners[p], pres[p][1], precision, x_in)
        print("%s pool %d (stride %d): %d winner flips of %d windows" % (label, p, layers[p].stride, n, winners[p].size))
    over = over_the_floor(label, m, layers, convs, precision, B, grads, want, floor, pres)
    assert all(float(g.abs().sum()) > 0 for g in grads.values())
    assert not over, (label, "(conv, rms ratio, max ratio) over 4 x the float32 floor", over)


@pytest.mark.parametrize("precision,stem", [("fp32", 16), ("f16s3", 32)])
def test_full_gradients_hold_the_bits_of_neck_gradients(tmp_path, precision, stem):
    """The entries of full_gradients that the neck scope also has are neck_gradients' bits on a plan with the same fusions off (option
    keep_backbone_activations holds them and keeps a superset of the neck's activations)."""
    m, t = _full_trainer(tmp_path, 64, 64, precision, stem)
    xd, bnd = _batch(64, 64)
    loss, heads, grads = t.full_gradients(xd, bnd)
    mn, tn = _full_trainer(tmp_path, 64, 64, precision, stem, name="n", trainable="neck", options={"keep_head_inputs": 1, "keep_backbone_activations": 1})
    loss_n, heads_n, neck = tn.neck_gradients(xd, bnd)
    assert sorted(neck) == [8, 9, 10, 14, 17] and _same(loss, loss_n)
    assert all(_same(grads[k], neck[k]) for k in neck) and all(_same(heads[k][0], heads_n[k][0]) and _same(heads[k][1], heads_n[k][1]) for k in heads_n)
    _, _, same_scope = t.neck_gradients(xd, bnd)                       # ... and on the full plan itself
    assert all(_same(same_scope[k], neck[k]) for k in neck)


def test_the_loss_falls_along_the_full_gradient_by_what_it_says(tmp_path):
    """scope_grad_cases.check_directional_derivative over all nine BatchNorm convs of pool_train_mini_cfg(64, 64), fp32, moved together;
    eps and the allowed gap come from the CPU model of the full sub-graph with torch's own leaky_relu and pools."""
    B = 3
    m, t = _full_trainer(tmp_path, 64, 64, "fp32", 16)
    xd, bnd = _batch(64, 64)
    _, _, grads = t.full_gradients(xd, bnd)
    l0 = float(t.last_components[0].item())
    assert sorted(grads) == POOL_MINI_FULL[16]
    images = full_batch(64, 64, 3, B)
    check_directional_derivative(m, t, xd, bnd, grads, cpu_scope_loss(m, t, B, images, grads, "full", t._net_input), l0)


@pytest.mark.parametrize("precision,stem", [("fp32", 16), ("f16s3", 32)])
def test_training_step_on_the_full_graph(tmp_path, precision, stem):
    """feed_forward_through_model(trainable="full"), an SGD step and then two Adam steps (scope_grad_cases.check_training_steps): masters
    and moments equal the torch expressions bit for bit, the packed image equals a fresh host pack of the synchronised stream.  With
    stem = 16 layer 0 (fp32 panel, 3 channels per tap padded to 4) and the Cin = 16 conv are among the stepped convs."""
    m, t = _full_trainer(tmp_path, 64, 64, precision, stem)
    xd, bnd = _batch(64, 64)
    trained = POOL_MINI_FULL[stem]
    assert (0 in trained and 2 in trained) == (stem == 16)
    check_training_steps(m, t, xd, bnd, "full", sorted(trained + [11, 18]), trained, [trained[0], 2])


def test_tiny_trains_all_eleven_convs(tmp_path):
    """YOLOv3-tiny itself at 416 x 416, batch 1, fp32: full_gradients returns a finite, nonzero dW for all 11 BatchNorm convs with the
    shapes of the module's weights, and one feed_forward_through_model step leaves the next forward finite."""
    text = cfgs.yolov3_tiny_cfg(416, 416)
    m, t = scope_trainer(tmp_path, text, 416, "fp32", trainable="full", options=FULL)
    xd = torch.from_numpy(synth.synth_frames(1, 416, seed=12)).cuda()
    bnd = [torch.from_numpy(full_batch(416, 416, 80, 1)[0])]
    _forward(m, xd)
    tenth_heads(m)
    assert [c for c, _ in m.full_layers()] == TINY_FULL
    loss, _, grads = t.full_gradients(xd, bnd)
    assert sorted(grads) == TINY_FULL and bool(torch.isfinite(loss))
    for c, dw in grads.items():
        w = next(sub for name, sub in m.module_list[c].named_children() if name.startswith("conv_")).weight
        assert tuple(dw.shape) == tuple(w.shape) and bool(torch.isfinite(dw).all()) and float(dw.abs().sum()) > 0, c
    t.optimizer = T.HeadOptimizer("adam", lr=1e-5)
    t.feed_forward_through_model(xd, bnd)
    assert bool(torch.isfinite(_forward(m, xd)).all()) and bool(torch.isfinite(t.forward_loss(xd, bnd)))
