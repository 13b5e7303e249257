"""GPU tests of the detection-block training path: rtod_conv_wgrad (csrc/wgrad.hip) and rtod_conv1x1_dgrad (csrc/dgrad.hip) against
exact integer and float64 sums, rtod_plan_step_conv_folded / rtod_plan_update_conv_weight against the host pack bit for bit, option
keep_block_inputs, and DarknetTrainer.block_gradients / feed_forward_through_model(trainable="blocks") end to end.

Gates, with u = 2^-24.
* Integers: operands in [-4, 4] make every product and partial sum an integer far below 2^24 (the slope 0.5 a half-integer), so
  the results equal the int64 sums bit for bit in any order.
* wgrad on floats: |dW - float64 sum| <= (K - 1) u sum |dz| |x| per element, K = B * H * W, the bound of a K-term fp32 sum (taps
  outside the map are exact zeros and count among the K terms).  For K = 1 that bound is 0, which no float32 result of an inexact
  product can meet: there the test asks for the correctly rounded product bit for bit (tests/test_head_grad_gpu.py's convention).
  With a row scale s the result is fl32(fl64(S~ s)) of the computed sum S~: |result - S s| <= (K - 1) u sum |s| + u' |S~ s| with
  |S~| <= (1 + (K - 1) u) sum and u' = u + 2^-53 (1 + u) for the double product's own rounding, so one more u:
  (K u + (K - 1) u^2 + 2^-52) sum |dz| |x| |s|, the last term covering 2^-53 (1 + u) (1 + (K - 1) u).  db likewise with |x| = 1
  (never scaled).
* dgrad on floats: one fmaf chain over Cout terms, then one multiplication: |dx - float64| <= (Cout + 1) u |m| sum_o |w| |dz|.
* Folded step: identical bits — masters and moments against block_grad_cases.opt_update_f32, the packed image as uint32 words.
* End to end: the docstrings of the tests."""
import functools

import numpy as np
import pytest
import torch

import head_opt_cases as A
from block_grad_cases import U, WGRAD_SHAPES, dgrad_ref, opt_update_f32, wgrad_ref
from head_grad_cases import conv_stream_ranges, cpu_head_model, pack
from loss_cases import bits
from scope_grad_cases import GATES, KEEP, _bn_of, _conv_of, _dev, _forward, _frames, _model, _same, _t64, scope_trainer, step_batch, tenth_heads
from scope_grad_cases import check_directional_derivative
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import HeadOptimizer

pytestmark = pytest.mark.gpu
F = np.float32
KEEP = KEEP["blocks"]


# ------------------------------------------------------------------------------------------ 1 / 2. the weight gradient
# WGRAD_SHAPES (block_grad_cases.py): the shapes the issue names and shapes chosen from the slice rule; the host test
# test_wgrad_shapes_span_the_slice_rule holds them to the slice counts the library itself reports
def _wgrad(dz, x, size, scale=None, bias=True):
    dw, db = T.conv_wgrad_async(_dev(dz), _dev(x), size, row_scale=None if scale is None else _dev(scale), bias=bias)
    return dw.cpu().numpy(), None if db is None else db.cpu().numpy()


@pytest.mark.parametrize("size", [3, 1])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv_wgrad_exact_on_small_integers(shape, size):
    B, cout, cin, H, W = shape
    rng = np.random.default_rng(B * 1000 + H * W + size)
    dz, x = rng.integers(-4, 5, (B, cout, H, W)), rng.integers(-4, 5, (B, cin, H, W))
    assert 16 * B * H * W < 2 ** 24
    dw, db = _wgrad(dz.astype(F), x.astype(F), size)
    want = wgrad_ref(dz, x, size, np.int64)
    assert dw.shape == (cout, cin, size, size) and np.array_equal(dw.astype(np.int64), want) and np.array_equal(dw, np.rint(dw)), (shape, size)
    assert np.array_equal(db.astype(np.int64), dz.sum(axis=(0, 2, 3))), (shape, size)
    if H == 1 and W == 1 and size == 3:                               # only the centre tap sees the pixel: the other eight are exactly 0
        off = np.ones((3, 3), bool)
        off[1, 1] = False
        assert not dw[:, :, off].any() and dw[:, :, 1, 1].any()
    # power-of-two row scales keep the integers exact
    s = 2.0 ** rng.integers(-3, 4, cout).astype(np.float64)
    dws, dbs = _wgrad(dz.astype(F), x.astype(F), size, scale=s)
    assert np.array_equal(dws.astype(np.float64), want * s[:, None, None, None]) and np.array_equal(dbs, db), (shape, size)


@pytest.mark.parametrize("size", [3, 1])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv_wgrad_floats_within_the_summation_bound_and_reproducible(shape, size):
    B, cout, cin, H, W = shape
    K = B * H * W
    rng = np.random.default_rng(B * 77 + H * W + size)
    dz, x = rng.standard_normal((B, cout, H, W)).astype(F), rng.standard_normal((B, cin, H, W)).astype(F)
    s = (rng.uniform(0.2, 3.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float64)
    dw, db = _wgrad(dz, x, size)
    dws, dbs = _wgrad(dz, x, size, scale=s)
    want = wgrad_ref(dz, x, size, np.float64)
    mass = wgrad_ref(np.abs(dz), np.abs(x), size, np.float64)
    s4 = s[:, None, None, None]
    if K == 1:                                                        # the bound is 0: the correctly rounded product, bit for bit ...
        assert np.array_equal(bits(dw), bits(want.astype(F))), (shape, size)
        assert np.array_equal(bits(dws), bits((want.astype(F).astype(np.float64) * s4).astype(F))), (shape, size)   # ... and its one scaling
    else:
        assert (np.abs(dw - want) <= (K - 1) * U * mass).all(), (shape, size, float((np.abs(dw - want) / np.maximum((K - 1) * U * mass, 1e-300)).max()))
        assert (np.abs(dws - want * s4) <= (K * U + (K - 1) * U * U + 2.0 ** -52) * mass * np.abs(s4)).all(), (shape, size)
    want_b, mass_b = dz.astype(np.float64).sum(axis=(0, 2, 3)), np.abs(dz).astype(np.float64).sum(axis=(0, 2, 3))
    assert (np.abs(db - want_b) <= (K - 1) * U * mass_b).all() and np.array_equal(bits(db), bits(dbs)), (shape, size)
    dw2, db2 = _wgrad(dz, x, size)
    dws2, _ = _wgrad(dz, x, size, scale=s, bias=False)
    assert dw.tobytes() == dw2.tobytes() and db.tobytes() == db2.tobytes() and dws.tobytes() == dws2.tobytes(), (shape, size)


# ------------------------------------------------------------------------------------------ 3. the data gradient
DGRAD_SHAPES = [(1, 1, 32, 1), (2, 18, 32, 4), (3, 255, 96, 169), (2, 255, 64, 35)]     # (B, Cout, Cin, P)


def _dgrad(w, dz, y, slope):
    B, cout, P = dz.shape
    dx = T.conv1x1_dgrad_async(_dev(w), _dev(dz).view(B, cout, P, 1), None if y is None else _dev(y).view(B, w.shape[1], P, 1), slope)
    return dx.cpu().numpy().reshape(B, w.shape[1], P)


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_dgrad_exact_on_small_integers(shape):
    B, cout, cin, P = shape
    rng = np.random.default_rng(B * 1000 + P)
    w, dz, y = rng.integers(-4, 5, (cout, cin)), rng.integers(-4, 5, (B, cout, P)), rng.integers(-1, 2, (B, cin, P))
    want = dgrad_ref(w, dz, np.int64).astype(np.float64)
    dx = _dgrad(w.astype(F), dz.astype(F), y.astype(F), 0.5)
    assert np.array_equal(dx.astype(np.float64), want * np.where(y > 0, 1.0, 0.5)), shape      # y == 0 takes the slope
    assert np.array_equal(_dgrad(w.astype(F), dz.astype(F), None, 0.5).astype(np.float64), want), shape          # no y: linear
    assert np.array_equal(_dgrad(w.astype(F), dz.astype(F), y.astype(F), 1.0).astype(np.float64), want), shape   # slope 1: linear


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_dgrad_floats_within_the_summation_bound_and_reproducible(shape):
    B, cout, cin, P = shape
    rng = np.random.default_rng(B * 77 + P)
    w, dz, y = (rng.standard_normal(s).astype(F) for s in ((cout, cin), (B, cout, P), (B, cin, P)))
    y[0, 0, 0] = 0.0
    slope = F(0.1)
    m = np.where(y > 0, 1.0, float(slope))
    dx = _dgrad(w, dz, y, float(slope))
    want = m * dgrad_ref(w, dz, np.float64)
    bound = (cout + 1) * U * m * dgrad_ref(np.abs(w), np.abs(dz), np.float64)
    assert (np.abs(dx - want) <= bound).all(), (shape, float((np.abs(dx - want) / bound).max()))
    assert dx.tobytes() == _dgrad(w, dz, y, float(slope)).tobytes(), shape


# ------------------------------------------------------------------------------------------ 4. the folded step is the host pack
BLOCKS = ((13, 1024, 512), (21, 512, 256))                           # mini_cfg(64, 64): block conv layer, Cout, Cin (both 3x3)


def _edited_image(m, text, res):
    """The packed image of the model's parameters as they are (masters synchronised into conv.weight, BatchNorm untouched), packed on the host."""
    stream = m.weight_stream().copy()
    return stream, pack(m._plan, stream)


@pytest.mark.parametrize("precision,sliced", [("fp32", 0), ("f16s3", 0), ("f16", 0), ("f16s3", 1), ("f16", 1)])
def test_folded_step_is_the_host_pack_and_the_documented_step_bit_for_bit(tmp_path, precision, sliced):
    """On both block convs of mini_cfg: an SGD step with lr = 0 on adversarial masters (tests/head_opt_cases.adversarial_head over the
    Cin * 9 columns of a row: an all-zero channel, power-of-two maxima, a 2^-45 and a 2^30 channel, negative zeros), an SGD step and
    three Adam steps with random gradients of either sign over six decades, then the host twin.  After the lr = 0 step, the SGD step,
    the last Adam step and the host twin the device image equals the host pack of the edited stream (the masters in conv.weight,
    BatchNorm as loaded) as uint32 words — the whole image: bias slots, padding and every other conv included — and after every
    step masters and moments equal block_grad_cases.opt_update_f32.  ``sliced``: the same on plans with option k_slices_split, where
    both block convs are K-sliced layers (conv_ks_f16s3.hip reads the blocks the step wrote) and still count as blocks."""
    res, B = 64, 2
    text = cfgs.mini_cfg(res, res)
    options = dict(KEEP, k_slices_split=1) if sliced else KEEP
    m = _model(tmp_path, text, res, precision, options)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=3)).cuda()
    before = _forward(m, x)
    assert m.active_precision == precision and m.head_blocks() == [(14, 13, 12), (22, 21, 20)]
    layers = m.plan_description()["layers"]
    assert [layers[b].get("k_slices", 0) > 1 for b in (13, 21)] == [bool(sliced)] * 2
    start = m.weight_stream().copy()
    ranges = conv_stream_ranges(build_ir(parse_cfg_text(text), res))
    rng = np.random.default_rng(41)
    state = {}
    for k, (layer, cout, cin) in enumerate(BLOCKS):
        w = A.adversarial_head(cout, cin * 9, 200 + k)[0]
        wd = _dev(w).view(cout, cin, 3, 3)
        dw = (rng.standard_normal(w.shape) * 10.0 ** rng.uniform(-3, 3, w.shape)).astype(F)
        dw[np.signbit(w) & (w == 0)] = np.abs(dw[np.signbit(w) & (w == 0)])                  # (-0) - (-0) = +0: the test is about the pack
        m.step_conv_folded(layer, _ffi.OptStep(0, 0.0, 0, 0, 0, 0), wd, _dev(dw).view(cout, cin, 3, 3))
        assert np.array_equal(bits(wd.cpu().numpy().reshape(cout, -1)), bits(w)), layer
        state[layer] = [wd, w, np.zeros_like(w), np.zeros_like(w), torch.zeros_like(wd), torch.zeros_like(wd)]
    stream, want = _edited_image(m, text, res)
    image = m.packed_weights()
    diff = np.flatnonzero(image != want)
    assert diff.size == 0, (precision, "pack", diff[:8].tolist(), diff.size)
    for layer, cout, cin in BLOCKS:                                   # the stream holds the masters, and BatchNorm is as it was
        off, n, bn = ranges[layer]
        assert bn and np.array_equal(bits(stream[off + 4 * cout:off + n]), bits(state[layer][1].reshape(-1))) and np.array_equal(bits(stream[off:off + 4 * cout]), bits(start[off:off + 4 * cout]))
    for step, kind in enumerate(["sgd", "adam", "adam", "adam"]):
        for layer, cout, cin in BLOCKS:
            wd, w, mm, vv, md, vd = state[layer]
            g = (rng.standard_normal(w.shape) * 10.0 ** rng.uniform(-3, 3, w.shape)).astype(F)
            if kind == "sgd":
                m.step_conv_folded(layer, _ffi.OptStep(0, 1e-3, 0, 0, 0, 0), wd, _dev(g).view(cout, cin, 3, 3))
                w1, m1, v1 = opt_update_f32("sgd", w, g, mm, vv, 1e-3)
            else:
                m.step_conv_folded(layer, _ffi.OptStep(1, A.LR, A.BETAS[0], A.BETAS[1], A.EPS, step), wd, _dev(g).view(cout, cin, 3, 3), (md, vd))
                w1, m1, v1 = opt_update_f32("adam", w, g, mm, vv, A.LR, A.BETAS, A.EPS, step)
            for name, dev_t, host in (("w", wd, w1), ("m", md, m1), ("v", vd, v1)):
                assert np.array_equal(bits(dev_t.cpu().numpy().reshape(cout, -1)), bits(host)), (precision, layer, kind, step, name)
            state[layer][1:4] = [w1, m1, v1]
        if step in (0, 3):                                            # after the SGD step and after the last Adam step
            stream, want = _edited_image(m, text, res)
            diff = np.flatnonzero(m.packed_weights() != want)
            assert diff.size == 0, (precision, kind, step, diff[:8].tolist(), diff.size)
    after = _forward(m, x)
    fresh = _model(tmp_path, text, res, precision, options, weights=stream, name="fresh")
    assert np.array_equal(bits(after.cpu().numpy()), bits(_forward(fresh, x).cpu().numpy())) and not _same(after, before)
    assert np.array_equal(fresh.packed_weights(), m.packed_weights())
    # the host twin: other weights through update_conv_weight, the bits of a full load of that stream
    version = (m._weights_version, m._plan_weights_version)
    for layer, cout, cin in BLOCKS:
        m.update_conv_weight(layer, torch.from_numpy(state[layer][1].reshape(cout, cin, 3, 3) * F(0.75)))
    assert (m._weights_version, m._plan_weights_version) == version   # no full re-pack is due
    stream, want = _edited_image(m, text, res)
    assert np.array_equal(m.packed_weights(), want)
    again = _model(tmp_path, text, res, precision, options, weights=stream, name="again")
    assert np.array_equal(bits(_forward(m, x).cpu().numpy()), bits(_forward(again, x).cpu().numpy())) and np.array_equal(again.packed_weights(), want)


# ------------------------------------------------------------------------------------------ 5. keep_block_inputs alone
@pytest.mark.parametrize("net,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "f16", None), ("mini", "fp32", 96), ("mini", "f16s3", 96),
                                                 ("tiny", "fp32", None), ("fallback", "fp32", None)])
def test_keep_block_inputs_changes_no_output_bit(tmp_path, net, precision, width):
    res, B = 64, 3
    text = {"mini": cfgs.mini_cfg, "tiny": cfgs.yolov3_tiny_cfg, "fallback": cfgs.mini_fallback_cfg}[net](res, width or res)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=6)).cuda() if width is None else torch.from_numpy(np.random.default_rng(6).random((B, 3, res, width)).astype(F)).cuda()
    off = _model(tmp_path, text, res, precision, name="off")
    on = _model(tmp_path, text, res, precision, {"keep_block_inputs": 1}, name="on")
    every = _model(tmp_path, text, res, precision, keep_all=True, name="all")
    for model in (off, on, every):
        model.input_width = width                                     # None: square; 96: the 96 wide x 64 high input
    for td in (False, True):
        y_off, y_on, y_all = _forward(off, x, td), _forward(on, x, td), _forward(every, x, td)
        assert np.array_equal(bits(y_off.cpu().numpy()), bits(y_on.cpu().numpy())) and np.array_equal(bits(y_off.cpu().numpy()), bits(y_all.cpu().numpy()))
        for _, block, inp in on.head_blocks():
            if block >= 0:
                got, want = on.read_layer(inp, B), every.read_layer(inp, B)
                assert got.abs().sum() > 0 and torch.equal(got, want), (net, precision, inp)
    assert [b for _, b, _ in on.head_blocks()] == {"mini": [13, 21], "tiny": [14, 21], "fallback": [-1, -1]}[net]
    assert [li.variant for li in off.launch_infos()] == [li.variant for li in on.launch_infos()]
    assert on._info.arena_bytes >= off._info.arena_bytes


# ------------------------------------------------------------------------------------------ 6. block_gradients against autograd
_block_trainer = functools.partial(scope_trainer, trainable="blocks", options=KEEP)


@pytest.mark.parametrize("net,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "fp32", 96), ("mini", "f16s3", 96), ("tiny", "fp32", None)])
def test_block_gradients_against_autograd(tmp_path, net, precision, width):
    """dW of DarknetTrainer.block_gradients against torch float64 autograd of the tail of the network, built here from the module's
    parameters: conv2d(x, W1) -> eval BatchNorm -> leaky(0.1) -> conv2d(., W2), fed the device's block input x (read_layer) and pulled
    back from the device's dz (rtod_yolo_loss_grad of the same forward).  requires_grad on W1 alone.

    The mask.  The device takes the leaky-ReLU derivative from the sign of its STORED block output; the float64 forward may put a
    pre-activation near zero on the other side.  Such a flip is legitimate only where |pre_64| is within the forward's own error:
      fp32    (K1 + 2) u (sum |w s| |x| + |bias|), K1 = Cin * k * k: one rounding of the folded weight, a K1-term fp32 sum, the bias;
      f16s3   1e-4 (sum |w s| |x| + |bias|), f16: 1e-3 — the project's parity gates of those precisions.
    A flip anywhere else fails the test.  The reference then uses the DEVICE's mask (leaky written as a product with that mask).

    The gate per element of dW1, with K = B * H * W, s the frozen scale, dy = m * W2^T dz:
      dgrad   |dy_dev - dy_64| <= E = (Cout2 + 1) u |m| sum_o |w2| |dz|                        (the float dgrad test's gate)
      wgrad   |S~ - sum dy_dev x| <= (K - 1) u sum |dy_dev| |x|,  |dy_dev| <= |dy_64| + E       (the float wgrad test's gate)
      scale   one more u on the result
      |dW_dev - dW_64| <= |s| ((1 + (K - 1) u) sum E |x| + (K - 1) u sum |dy_64| |x|) (1 + u) + u |dW_64|."""
    res, B = 64, 3
    text = cfgs.mini_cfg(res, width or res) if net == "mini" else cfgs.yolov3_tiny_cfg(res, res)
    m, t = _block_trainer(tmp_path, text, res, precision, width)
    xd = _frames(B, res, width)
    _, images = step_batch()
    bnd = [torch.from_numpy(im) for im in images]
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, block_grads = t.block_gradients(xd, bnd)
    blocks = m.head_blocks()
    assert m.active_precision == precision and int(t.status.item()) == 0
    assert blocks == ([(14, 13, 12), (22, 21, 20)] if net == "mini" else [(15, 14, 13), (22, 21, 20)]) and sorted(block_grads) == [b for _, b, _ in blocks]
    # the heads' part is head_gradients, bit for bit
    loss_h, grads_h = t.head_gradients(xd, bnd)
    assert _same(loss, loss_h) and all(_same(head_grads[k][0], grads_h[k][0]) and _same(head_grads[k][1], grads_h[k][1]) for k in grads_h)
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    fn = torch.nn.functional
    for (head, block, inp), dz in zip(blocks, dzs):
        conv, bn, size = _conv_of(m, block), _bn_of(m, block), _conv_of(m, block).kernel_size[0]
        x, y_dev = _t64(m.read_layer(inp, B)), m.read_layer(block, B).cpu().numpy()
        W1 = _t64(conv.weight).requires_grad_(True)
        W2, dz64 = _t64(_conv_of(m, head).weight), _t64(dz)
        gamma, beta, mean, var = (_t64(v) for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        pre = fn.batch_norm(fn.conv2d(x, W1, padding=size // 2), mean, var, gamma, beta, False, 0.0, 1e-5)
        mask_dev = torch.from_numpy(np.where(y_dev > 0, 1.0, 0.1))
        fn.conv2d(pre * mask_dev, W2).backward(dz64)
        want = W1.grad.numpy()
        # the mask
        s = (gamma / torch.sqrt(var + 1e-5)).numpy()
        shift = (beta.numpy() - mean.numpy() * s)
        mass = fn.conv2d(x.abs(), (W1.detach() * torch.from_numpy(s)[:, None, None, None]).abs(), padding=size // 2).numpy() + np.abs(shift)[None, :, None, None]
        K1 = conv.in_channels * size * size
        gate = (K1 + 2) * U * mass if GATES[precision] is None else GATES[precision] * mass
        flips = (pre.detach().numpy() > 0) != (y_dev > 0)
        assert (np.abs(pre.detach().numpy())[flips] <= gate[flips]).all(), (net, precision, block, int(flips.sum()))
        # the gradient
        m_dev = mask_dev.numpy()
        w2 = W2.numpy()[:, :, 0, 0]
        Bn, _, H, Wd = dz.shape
        flat = lambda a: a.reshape(Bn, a.shape[1], H * Wd)
        dy64 = (m_dev * dgrad_ref(w2, flat(dz64.numpy()), np.float64).reshape(m_dev.shape))
        E = (w2.shape[0] + 1) * U * m_dev * dgrad_ref(np.abs(w2), np.abs(flat(dz64.numpy())), np.float64).reshape(m_dev.shape)
        K = Bn * H * Wd
        xa = np.abs(x.numpy())
        s4 = np.abs(s)[:, None, None, None]
        bound = s4 * ((1 + (K - 1) * U) * wgrad_ref(E, xa, size, np.float64) + (K - 1) * U * wgrad_ref(np.abs(dy64), xa, size, np.float64)) * (1 + U) + U * np.abs(want)
        assert np.allclose(want, s[:, None, None, None] * wgrad_ref(dy64, x.numpy(), size, np.float64), rtol=1e-9, atol=1e-12 * np.abs(want).max())   # autograd is the chain above
        got = block_grads[block].cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print("%s %s block %d (K = %d, %d flips): worst error / bound %.3g, max |dW| %.3g" % (net, precision, block, K, int(flips.sum()),
              float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()), float(np.abs(want).max())))
        assert got.shape == want.shape and np.abs(want).max() > 0 and (err <= bound).all(), (net, precision, block)


# ------------------------------------------------------------------------------------------ 7. the directional derivative
def _cpu_loss(m, t, xs, W1s, images, dtype):
    """The loss of the two-conv tails on the CPU in ``dtype`` (None: float64) as a function of the block weights W1s, on the block inputs xs."""
    dt = torch.float64 if dtype is None else dtype
    fn = torch.nn.functional
    cast = lambda a: torch.as_tensor(np.asarray(a), dtype=dt)
    acts, ws, bs = [], [], []
    for (head, block, _), x, W1 in zip(m.head_blocks(), xs, W1s):
        bn, size = _bn_of(m, block), _conv_of(m, block).kernel_size[0]
        pre = fn.batch_norm(fn.conv2d(cast(x), cast(W1), padding=size // 2), cast(_t64(bn.running_mean)), cast(_t64(bn.running_var)),
                            cast(_t64(bn.weight)), cast(_t64(bn.bias)), False, 0.0, 1e-5)
        acts.append(fn.leaky_relu(pre, 0.1).numpy())
        ws.append(_t64(_conv_of(m, head).weight).numpy())
        bs.append(_t64(_conv_of(m, head).bias).numpy())
    if dtype is not None:
        ws, bs = [a.astype(F) for a in ws], [a.astype(F) for a in bs]
    return cpu_head_model(acts, ws, bs, t.heads, images, 4, dtype)["loss"]


def test_the_loss_falls_along_the_block_gradient_by_what_it_says(tmp_path):
    """The central difference of the device loss along -g, (L(W1 + eps g) - L(W1 - eps g)) / (2 eps) with the block weights moved by
    update_conv_weight, against ||g||^2 of block_gradients (fp32 plan, mini_cfg(64, 64), the batch of step_batch), in the manner of
    test_the_step_descends_by_what_the_gradient_says.

    eps and the allowed gap come from a float64 CPU model of the two-conv tails on the device's own block inputs (_cpu_loss), never
    from a device result: along the same direction g the model's central difference misses its own derivative by a truncation term
    that falls as eps^2, and the loss evaluated in float32 differs from the float64 loss by `noise`, which a difference quotient
    divides by eps.  eps is the smallest of 1e-2, 3e-3, 1e-3, ... at which the modelled truncation gap still exceeds that noise term
    tenfold, so that the allowed gap is a figure the model predicts rather than noise; the test allows
        4 * |fd_cpu - dd_cpu|  +  2 * noise / (2 eps),      dd_cpu the model's central difference at a tenth of eps,
    the convention of that test (4 x for an equally legitimate arrangement of the roundings, one noise per loss evaluation; noise
    here is the largest float32 - float64 difference of the model at the three points 0, +eps, -eps)."""
    B = 3
    m, t = _block_trainer(tmp_path, cfgs.mini_cfg(64, 64), 64, "fp32")
    x, images = step_batch()
    xd, bnd = torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images]
    loss0, _, grads = t.block_gradients(xd, bnd)
    l0 = float(t.last_components[0].item())
    blocks = m.head_blocks()
    xs = [m.read_layer(inp, B).cpu().numpy().astype(np.float64) for _, _, inp in blocks]
    W1s = [_t64(_conv_of(m, b).weight).numpy() for _, b, _ in blocks]
    gs = [grads[b].cpu().numpy().astype(np.float64) for _, b, _ in blocks]
    cpu = lambda s, dtype: _cpu_loss(m, t, xs, [w + s * g for w, g in zip(W1s, gs)], images, None if dtype == torch.float64 else dtype)
    check_directional_derivative(m, t, xd, bnd, grads, cpu, l0)


# ------------------------------------------------------------------------------------------ 8. the training step
def _batch():
    x, images = step_batch()
    return torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images]


@pytest.mark.parametrize("precision,width", [("fp32", None), ("f16s3", None), ("f16s3", 96)])
def test_training_step_on_blocks(tmp_path, precision, width):
    """feed_forward_through_model(trainable="blocks"): every gradient is taken before the first step (an SGD step equals the documented
    step applied to block_gradients of an identical model), the next forward and a graph captured BEFORE the steps run the stepped
    weights, a fresh model built from state_dict() computes the same bits, the optimiser's state carries a second trainer on, and
    trainable="heads" is untouched by the new options.  ``width``: None for the square 64x64 input, 96 for 96 wide x 64 high."""
    text = cfgs.mini_cfg(64, width or 64)
    xd, bnd = _frames(3, 64, width), _batch()[1]
    # heads alone: the plan options of the block path change nothing, and the block convs stay as they were
    m0, t0 = _block_trainer(tmp_path, text, 64, precision, width, name="h0", trainable="heads", options={"keep_head_inputs": 1})
    m1, t1 = _block_trainer(tmp_path, text, 64, precision, width, name="h1", trainable="heads")
    l0, l1 = [t0.feed_forward_through_model(xd, bnd) for _ in range(2)], [t1.feed_forward_through_model(xd, bnd) for _ in range(2)]
    assert all(_same(a, b) for a, b in zip(l0, l1)) and np.array_equal(m0.packed_weights(), m1.packed_weights())
    assert sorted(t1.optimizer.state) == [14, 22] and sorted(t1.optimizer.state[14]) == ["bias", "exp_avg", "exp_avg_bias", "exp_avg_sq", "exp_avg_sq_bias", "step", "weight"]
    # one SGD step on blocks and heads: the documented step of the gradients of the unstepped model
    ma, ta = _block_trainer(tmp_path, text, 64, precision, width, name="a")
    mb, tb = _block_trainer(tmp_path, text, 64, precision, width, name="b")
    tb.optimizer = HeadOptimizer("sgd", lr=1e-4)
    loss_a, hg, bg = ta.block_gradients(xd, bnd)
    graph_run = mb.make_graphed(xd)                                   # captured before any step
    y_before = graph_run(xd)[0].clone()
    loss_b = tb.feed_forward_through_model(xd, bnd)
    assert _same(loss_a, loss_b) and _same(loss_b, l0[0]) and sorted(tb._head_masters) == [13, 14, 21, 22]
    for layer in (13, 21):
        w0 = _conv_of(ma, layer).weight.detach().numpy()
        want = opt_update_f32("sgd", w0, bg[layer].cpu().numpy(), None, None, 1e-4)[0]
        assert np.array_equal(bits(tb._head_masters[layer][0].cpu().numpy()), bits(want)) and tb._head_masters[layer][1] is None, layer
        assert not _same(_conv_of(mb, layer).weight, tb._head_masters[layer][0])       # the module's parameters lag behind
    for layer in (14, 22):
        want = opt_update_f32("sgd", _conv_of(ma, layer).weight.detach().numpy(), hg[layer][0].cpu().numpy(), None, None, 1e-4)[0]
        assert np.array_equal(bits(tb._head_masters[layer][0].cpu().numpy()), bits(want)), layer
    # the next forward, and the captured graph, run the stepped weights; a fresh model from state_dict() gives the same bits
    y = _forward(mb, xd)
    y_graph = graph_run(xd)[0]
    assert _same(y, y_graph) and not _same(y, y_before)
    sd = mb.state_dict()
    assert _same(sd["module_list.13.conv_13.weight"], tb._head_masters[13][0]) and _same(sd["module_list.22.conv_22.bias"], tb._head_masters[22][1])
    fresh = _model(tmp_path, text, 64, precision, KEEP, name="fresh")
    fresh.input_width = width
    fresh.load_state_dict(sd)
    assert _same(_forward(fresh, xd), y) and np.array_equal(fresh.packed_weights(), mb.packed_weights())
    # Adam (the default): three steps, then the state round trip carries a second trainer on
    mc, tc = _block_trainer(tmp_path, text, 64, precision, width, name="c")
    tc.optimizer.lr = 1e-4
    losses = [float(tc.feed_forward_through_model(xd, bnd)) for _ in range(3)]
    assert losses[0] == float(l0[0]) and np.isfinite(losses).all() and losses[1] != losses[0], losses
    state = tc.optimizer.state_dict()
    assert sorted(state) == [13, 14, 21, 22] and sorted(state[13]) == ["exp_avg", "exp_avg_sq", "step", "weight"] and state[13]["step"] == 3
    assert sorted(state[14]) == ["bias", "exp_avg", "exp_avg_bias", "exp_avg_sq", "exp_avg_sq_bias", "step", "weight"]
    md, td = _block_trainer(tmp_path, text, 64, precision, width, name="d")
    td.optimizer.lr = 1e-4
    td.optimizer.load_state_dict(state)
    assert td.optimizer.state[13]["weight"] is not state[13]["weight"] and td._head_masters[13][0] is td.optimizer.state[13]["weight"] and td._head_masters[13][1] is None
    la, lb = tc.feed_forward_through_model(xd, bnd), td.feed_forward_through_model(xd, bnd)
    assert _same(la, lb)
    for layer in (13, 14, 21, 22):
        for k in state[layer]:
            if k != "step":
                assert _same(tc.optimizer.state[layer][k], td.optimizer.state[layer][k]), (layer, k)
        assert tc.optimizer.state[layer]["step"] == td.optimizer.state[layer]["step"] == 4
    assert np.array_equal(mc.packed_weights(), md.packed_weights())
