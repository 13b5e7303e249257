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
import numpy as np
import pytest
import torch

from block_grad_cases import opt_update_f32
from head_grad_cases import cpu_head_model, pack
from loss_cases import bits
from neck_grad_cases import DGRAD_SHAPES, NECK, U, UPSAMPLE_SHAPES, conv_dgrad_ref
from test_block_grad_gpu import GATES, _bn_of, _frames, _t64
from test_head_grad_gpu import _conv_of, _forward, _model, step_batch
from realtimeobjectdetection_amd import cfgs, train as T
from realtimeobjectdetection_amd.train import HeadOptimizer

pytestmark = pytest.mark.gpu
F = np.float32
KEEP = {"keep_head_inputs": 1, "keep_neck_activations": 1}
fn = torch.nn.functional


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))


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
def _neck_trainer(tmp_path, text, res, precision, width=None, name="m", trainable="neck", options=KEEP):
    m = _model(tmp_path, text, res, precision, options, name=name)
    if width is not None:
        m.input_width = width
    t = T.DarknetTrainer(m, trainable=trainable)
    t.min_box_size = 4
    return m, t


def _cpu_neck(m, t, B, dtype, weights=None, masks=None, cut=None):
    """The neck sub-graph on the CPU in ``dtype`` from the module's parameters: conv -> eval BatchNorm -> leaky (written as a product with
    ``masks[layer]``, the DEVICE's, where given; else torch's leaky_relu), routes, F.interpolate, head convs; fed the device's boundary
    inputs (read_layer of the layers the graph reads from outside).  ``weights``: {neck conv: weight} in place of the module's;
    ``cut = (producer, reader)``: that reader sees the producer's value detached (its contribution to the producer's gradient is zero).
    Returns (values per layer, {neck conv: leaf weight}, {neck conv: (pre-activation, input)})."""
    layers, readers, member, scales = t._neck()
    cast = lambda a: torch.as_tensor(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).to(dtype)
    val, leaves, pres = {}, {}, {}

    def value(src, reader):
        if src not in val:
            assert not member[src]
            val[src] = cast(m.read_layer(src, B))
        return val[src].detach() if cut == (src, reader) else val[src]

    for L in layers:
        i = L.index
        if not member[i]:
            continue
        if L.type == "convolutional":
            conv, x = _conv_of(m, i), value(i - 1, i)
            W = cast(conv.weight if weights is None or i not in weights else weights[i])
            if i in scales:
                W.requires_grad_(True)
                leaves[i] = W
                bn = _bn_of(m, i)
                pre = fn.batch_norm(fn.conv2d(x, W, padding=L.size // 2), cast(bn.running_mean), cast(bn.running_var), cast(bn.weight), cast(bn.bias), False, 0.0, 1e-5)
                pres[i] = (pre, x)
                val[i] = pre if not L.leaky else pre * cast(masks[i]) if masks is not None else fn.leaky_relu(pre, 0.1)
            else:
                val[i] = fn.conv2d(x, W, cast(conv.bias))
        elif L.type == "upsample":
            x = value(i - 1, i)
            val[i] = fn.interpolate(x, scale_factor=2, mode="nearest") if L.nearest else fn.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        else:                                                         # a source outside the graph: its slice of the kept concat buffer
            parts, off = [], 0
            for s in L.srcs:
                parts.append(value(s, i) if member[s] else cast(m.read_layer(i, B))[:, off:off + layers[s].cout])
                off += layers[s].cout
            val[i] = torch.cat(parts, 1)
    return val, leaves, pres


def _cpu_neck_grads(m, t, B, dtype, masks, dzs, cut=None):
    val, leaves, pres = _cpu_neck(m, t, B, dtype, masks=masks, cut=cut)
    total = sum((val[head] * dz.detach().cpu().to(dtype)).sum() for (head, _), dz in zip(m.head_layers(), dzs))
    total.backward()
    return {i: W.grad.numpy().astype(np.float64) for i, W in leaves.items()}, pres


@pytest.mark.parametrize("net,precision,width", [("mini", "fp32", None), ("mini", "f16s3", None), ("mini", "fp32", 96), ("tiny", "fp32", None)])
def test_neck_gradients_against_autograd(tmp_path, net, precision, width):
    """dW of DarknetTrainer.neck_gradients for every neck conv against torch autograd of the neck sub-graph (_cpu_neck) with the DEVICE's
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
    for head, _ in m.head_layers():                                   # a tenth of the synthetic head weights: sigmoids that do not saturate
        m.update_conv(head, _conv_of(m, head).weight.detach() * 0.1, _conv_of(m, head).bias.detach() * 0.1)
    loss, head_grads, neck_grads = t.neck_gradients(xd, bnd)
    assert m.active_precision == precision and int(t.status.item()) == 0 and sorted(neck_grads) == NECK[net] == [c for c, _ in m.neck_layers()]
    # twice the same bytes; the heads' part is head_gradients; the block convs' entries are block_gradients of a "blocks" trainer
    loss2, _, again = t.neck_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(neck_grads[k], again[k]) for k in neck_grads)
    loss_h, grads_h = t.head_gradients(xd, bnd)
    assert _same(loss, loss_h) and all(_same(head_grads[k][0], grads_h[k][0]) and _same(head_grads[k][1], grads_h[k][1]) for k in grads_h)
    mb, tb = _neck_trainer(tmp_path, text, res, precision, width, name="blocks", trainable="blocks", options={"keep_head_inputs": 1, "keep_block_inputs": 1})
    _forward(mb, xd)
    for head, _ in mb.head_layers():
        mb.update_conv(head, _conv_of(mb, head).weight.detach() * 0.1, _conv_of(mb, head).bias.detach() * 0.1)
    loss_b, _, block_grads = tb.block_gradients(xd, bnd)
    assert _same(loss, loss_b) and len(block_grads) == len(m.head_layers()) and all(_same(neck_grads[k], block_grads[k]) for k in block_grads)
    # the CPU model with the device's masks
    layers, readers, member, scales = t._neck()
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in NECK[net] if layers[c].leaky}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    want, pres = _cpu_neck_grads(m, t, B, torch.float64, masks, dzs)
    floor, _ = _cpu_neck_grads(m, t, B, torch.float32, masks, dzs)
    over = []
    for c in NECK[net]:
        conv, bn, size = _conv_of(m, c), _bn_of(m, c), layers[c].size
        pre, x = (a.detach() for a in pres[c])
        gamma, beta, mean, var = (_t64(v) for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        s = (gamma / torch.sqrt(var + 1e-5))
        mass = fn.conv2d(x.abs(), (_t64(conv.weight) * s[:, None, None, None]).abs(), padding=size // 2).numpy() + np.abs((beta - mean * s).numpy())[None, :, None, None]
        gate = ((conv.in_channels * size * size + 2) * U if GATES[precision] is None else GATES[precision]) * mass
        y_dev = m.read_layer(c, B).cpu().numpy()
        flips = (pre.numpy() > 0) != (y_dev > 0)
        assert (np.abs(pre.numpy())[flips] <= gate[flips]).all(), (net, precision, c, int(flips.sum()))
        got, ref = neck_grads[c].cpu().numpy().astype(np.float64), np.abs(want[c]).max()
        assert got.shape == want[c].shape and ref > 0
        e_dev, e_32 = (got - want[c]) / ref, (floor[c] - want[c]) / ref
        rms = lambda e: float(np.sqrt(np.mean(e * e)))
        print("%s %s conv %d (%d flips): rms %.3g (float32 floor %.3g, ratio %.2f)  max %.3g (floor %.3g, ratio %.2f)" % (
            net, precision, c, int(flips.sum()), rms(e_dev), rms(e_32), rms(e_dev) / rms(e_32), np.abs(e_dev).max(), np.abs(e_32).max(), np.abs(e_dev).max() / np.abs(e_32).max()))
        if not (rms(e_dev) <= 4 * rms(e_32) and np.abs(e_dev).max() <= 4 * np.abs(e_32).max()):
            over.append((c, round(rms(e_dev) / rms(e_32), 2), round(float(np.abs(e_dev).max() / np.abs(e_32).max()), 2)))
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
    g2 = sum(float((dw.double() ** 2).sum()) for dw in grads.values())
    W0 = {c: _conv_of(m, c).weight.detach().clone() for c in grads}
    heads = [h for h, _ in m.head_layers()]

    def cpu(s, dtype=torch.float64):
        with torch.no_grad():
            val, _, _ = _cpu_neck(m, t, B, dtype, weights={c: W0[c].double() + s * grads[c].cpu().double() for c in grads})
        val = {k: v.detach() for k, v in val.items()}
        acts = [val[h - 1].numpy() for h in heads]
        ws = [_t64(_conv_of(m, h).weight).numpy() for h in heads]
        bs = [_t64(_conv_of(m, h).bias).numpy() for h in heads]
        if dtype != torch.float64:
            ws, bs = [a.astype(F) for a in ws], [a.astype(F) for a in bs]
        return cpu_head_model(acts, ws, bs, t.heads, images, 4, None if dtype == torch.float64 else dtype)["loss"]
    noise_at = lambda s: abs(cpu(s, torch.float32) - cpu(s))
    noise = noise_at(0.0)
    eps = gap_cpu = None
    for e in (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7):
        fd, dd = (cpu(e) - cpu(-e)) / (2 * e), (cpu(e / 10) - cpu(-e / 10)) / (2 * e / 10)
        if abs(fd - dd) >= 10 * noise / e:
            eps, gap_cpu = e, abs(fd - dd)
    assert eps is not None
    noise = max(noise, noise_at(eps), noise_at(-eps))
    allowed = 4 * gap_cpu + 2 * noise / (2 * eps)
    masters = {c: W0[c].cuda() for c in grads}

    def loss_at(s):
        for c in grads:
            m.update_conv_weight(c, masters[c] + s * grads[c])
        t.forward_loss(xd, bnd)
        return float(t.last_components[0].item())
    fd_dev = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
    assert loss_at(0.0) == l0                                         # the weights are back, bit for bit
    print("||g||^2 device %.8g; eps %.0e; central difference device %.8g; gap %.4g, allowed %.4g (cpu gap %.4g, noise %.4g)" % (g2, eps, fd_dev, abs(fd_dev - g2), allowed, gap_cpu, noise))
    assert g2 > 0 and abs(fd_dev - g2) <= allowed


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
    losses = []
    host = lambda a: None if a is None else a.detach().cpu().numpy()
    for step, kind in enumerate(["sgd", "adam", "adam"]):
        if step < 2:
            t.optimizer = HeadOptimizer(kind, lr=1e-4)
        _, hg, ng = t.neck_gradients(xd, bnd)
        grads = {k: (host(dw), host(db)) for k, (dw, db) in hg.items()}
        grads.update({k: (host(dw), None) for k, dw in ng.items()})
        assert sorted(grads) == layers
        masters = t._masters(grads, xd.device)
        before = {k: (host(masters[k][0]), host(masters[k][1])) for k in layers}
        state = {k: {n: host(v) for n, v in t.optimizer.state.get(k, {}).items() if n.startswith("exp_avg")} for k in layers}
        losses.append(float(t.feed_forward_through_model(xd, bnd)))
        for k in layers:
            st = t.optimizer.state[k]
            assert st["step"] == (1 if step < 2 else 2) and st["weight"] is t._head_masters[k][0]
            for which, name, sfx in ((0, "weight", ""), (1, "bias", "_bias")):
                if before[k][which] is None:
                    assert which == 1 and "bias" not in st and k in NECK["mini"]
                    continue
                zero = np.zeros_like(before[k][which])
                w1, m1, v1 = opt_update_f32(kind, before[k][which], grads[k][which], state[k].get("exp_avg" + sfx, zero), state[k].get("exp_avg_sq" + sfx, zero),
                                            1e-4, step=st["step"])
                assert np.array_equal(bits(host(st[name])), bits(w1)), (precision, step, k, name)
                if kind == "adam":
                    assert np.array_equal(bits(host(st["exp_avg" + sfx])), bits(m1)) and np.array_equal(bits(host(st["exp_avg_sq" + sfx])), bits(v1)), (precision, step, k, name)
        image = m.packed_weights()
        stream = m.weight_stream().copy()                             # synchronises the masters into the module's parameters
        assert _same(_conv_of(m, 12).weight, t._head_masters[12][0]) and np.array_equal(image, pack(m._plan, stream)), (precision, step)
    assert losses[1] != losses[0] and np.isfinite(losses).all(), losses
    # the block path on a twin: the same bits with and without the new option
    out = []
    for name, options in (("b0", {"keep_head_inputs": 1, "keep_block_inputs": 1}), ("b1", dict(KEEP, keep_block_inputs=1))):
        mb, tb = _neck_trainer(tmp_path, text, 64, precision, width, name=name, trainable="blocks", options=options)
        tb.optimizer.lr = 1e-4
        out.append(([tb.feed_forward_through_model(xd, bnd) for _ in range(2)], mb.packed_weights(), sorted(tb.optimizer.state)))
    assert all(_same(a, b) for a, b in zip(out[0][0], out[1][0])) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] == [13, 14, 21, 22]
    assert float(out[0][0][0]) == losses[0]
