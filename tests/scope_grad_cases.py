"""What the host and GPU tests of the training scopes (heads, blocks, neck, backbone, full) share: the plan's listing entries on the C ABI,
models and trainers on synthetic weights, the fixed batch of the end-to-end tests, the CPU model of a scope's sub-graph with its
autograd gradients, and the gate every end-to-end gradient test applies: the mask-flip rule and 4 x the float32 floor."""
import ctypes as C
import warnings

import numpy as np
import torch

from head_grad_cases import cpu_head_model, pack
from loss_cases import bits
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text

F = np.float32
U = 2.0 ** -24
fn = torch.nn.functional
GATES = {"fp32": None, "f16s3": 1e-4, "f16": 1e-3}                  # the forward's own error as a fraction of the mass; None: (K1 + 2) u
KEEP = {"blocks": {"keep_head_inputs": 1, "keep_block_inputs": 1}, "neck": {"keep_head_inputs": 1, "keep_neck_activations": 1},
        "backbone": {"keep_head_inputs": 1, "keep_backbone_activations": 1}, "full": {"keep_head_inputs": 1, "keep_full_activations": 1}}
ENTRY = {"blocks": "block_gradients", "neck": "neck_gradients", "backbone": "backbone_gradients", "full": "full_gradients"}


def plan_list(entry, h, columns):
    """rtod_plan_head_blocks (3 columns), rtod_plan_neck_layers or rtod_plan_trainable_layers (2) of plan handle ``h``: the count, then the rows."""
    call = getattr(_ffi.lib(), entry)
    n = call(h, *[None] * columns, 0)
    assert n >= 0
    arrs = [(C.c_int * max(n, 1))() for _ in range(columns)]
    assert call(h, *arrs, n) == n
    return list(zip(*[list(a)[:n] for a in arrs]))


# ---------------------------------------------------------------------------------------------- models, trainers, batches
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))


def _t64(a):
    return torch.as_tensor(a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64))


def _model(d, text, res, precision, options=None, train=False, keep_all=False, weights=None, name="m"):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / (name + ".cfg")), text), True)
    m = m.train() if train else m.eval()
    m.net_info["height"] = res
    m.precision = precision
    m.options = dict(options or {})
    m.keep_all_layers = keep_all
    m.update_running_stats = False
    m.autotune = False
    m.load_weight_stream(synth.synth_weights(build_ir(parse_cfg_text(text), res)) if weights is None else weights)
    return m


def _forward(m, x, train_decode=False):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # the training-mode warning of the batch-statistics plans
        if train_decode:
            with m.train_mode():
                return m(x)
        return m(x)


def _conv_of(m, layer):
    return next(sub for name, sub in m.module_list[layer].named_children() if name.startswith("conv_"))


def _bn_of(m, layer):
    return next(sub for name, sub in m.module_list[layer].named_children() if name.startswith("batch_norm_"))


def _frames(B, res, width):
    if width is None:
        return torch.from_numpy(synth.synth_frames(B, res, seed=12)).cuda()
    return torch.from_numpy(np.random.default_rng(12).random((B, 3, res, width)).astype(F)).cuda()


def _box(cx, cy, w, h, C_, cls=0):
    r = np.zeros(5 + C_, F)
    r[:5] = (cx, cy, w, h, 1.0)
    r[5 + cls] = 1.0
    return r


def step_batch(res=64, B=3):
    """The fixed batch of the end-to-end tests: synthetic frames and a few class-0 boxes per image (one image without boxes)."""
    x = synth.synth_frames(B, res, seed=12)
    images = [np.stack([_box(20, 22, 30, 26, 80), _box(45, 40, 24, 36, 80), _box(33, 50, 50, 18, 80)]), np.zeros((0, 85), F),
              np.stack([_box(10, 50, 12, 40, 80), _box(52, 12, 20, 20, 80, cls=2), _box(40, 30, 60, 60, 80)])][:B]
    return x, images


def scope_trainer(tmp_path, text, res, precision, width=None, name="m", trainable="blocks", options=None):
    """A model on synthetic weights with ``options`` (None: what ``trainable`` needs) and its trainer, boxes from 4 pixels on."""
    m = _model(tmp_path, text, res, precision, KEEP[trainable] if options is None else options, name=name)
    if width is not None:
        m.input_width = width
    t = T.DarknetTrainer(m, trainable=trainable)
    t.min_box_size = 4
    return m, t


def tenth_heads(m):
    for head, _ in m.head_layers():                                   # a tenth of the synthetic head weights: sigmoids that do not saturate
        m.update_conv(head, _conv_of(m, head).weight.detach() * 0.1, _conv_of(m, head).bias.detach() * 0.1)


# ---------------------------------------------------------------------------------------------- the CPU model of a scope's sub-graph
def torch_pool(x, stride):
    """The reference's two modules: nn.MaxPool2d(2, 2), and MaxPoolStride1 (replicate pad right / bottom, then MaxPool2d(2, 1))."""
    return fn.max_pool2d(x, 2, 2) if stride == 2 else fn.max_pool2d(fn.pad(x, (0, 1, 0, 1), mode="replicate"), 2, 1)


def cpu_graph(m, t, B, dtype, weights=None, masks=None, cut=None, *, scope, x_in=None, winners=None):
    """The sub-graph ``t._graph(scope)`` on the CPU in ``dtype`` from the module's parameters: conv (stride 1 or 2) -> eval BatchNorm ->
    leaky (written as a product with ``masks[layer]``, the DEVICE's, where given; else torch's leaky_relu), shortcuts, routes,
    F.interpolate, head convs, and a [maxpool] as a gather with ``winners[layer]`` (full_grad_cases.pool_winners of the DEVICE's
    read_layer copy of the pool's input) where given, else torch's own pool; fed the device's boundary inputs (read_layer of the layers
    the graph reads from outside) and ``x_in``, the prepared network input, where layer 0 is a member.  ``weights``: {conv: weight} in
    place of the module's; ``cut = (producer, reader)``: that reader sees the producer's value detached (its contribution to the
    producer's gradient is zero).  Returns (values per layer, {conv: leaf weight}, {conv: (pre-activation, input), pool: (None, input)})."""
    layers, readers, member, scales = t._graph(scope)
    cast = lambda a: torch.as_tensor(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).to(dtype)
    val, leaves, pres = ({} if x_in is None else {-1: cast(x_in)}), {}, {}

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
                pre = fn.batch_norm(fn.conv2d(x, W, stride=L.stride, padding=L.size // 2), cast(bn.running_mean), cast(bn.running_var), cast(bn.weight), cast(bn.bias),
                                    False, 0.0, 1e-5)
                pres[i] = (pre, x)
                val[i] = pre if not L.leaky else pre * cast(masks[i]) if masks is not None else fn.leaky_relu(pre, 0.1)
            else:
                val[i] = fn.conv2d(x, W, cast(conv.bias))
        elif L.type == "maxpool":
            x = value(i - 1, i)
            pres[i] = (None, x)
            if winners is None:
                val[i] = torch_pool(x, L.stride)
            else:
                idx = torch.from_numpy(winners[i])
                val[i] = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
        elif L.type == "upsample":
            x = value(i - 1, i)
            val[i] = fn.interpolate(x, scale_factor=2, mode="nearest") if L.nearest else fn.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        elif L.type == "shortcut":
            val[i] = value(L.srcs[0], i) + value(L.srcs[1], i)
        else:                                                         # a source outside the graph: its slice of the kept concat buffer
            parts, off = [], 0
            for s in L.srcs:
                parts.append(value(s, i) if member[s] else cast(m.read_layer(i, B))[:, off:off + layers[s].cout])
                off += layers[s].cout
            val[i] = torch.cat(parts, 1)
    return val, leaves, pres


def cpu_graph_grads(m, t, B, dtype, masks, dzs, cut=None, *, scope, x_in=None, winners=None):
    val, leaves, pres = cpu_graph(m, t, B, dtype, masks=masks, cut=cut, scope=scope, x_in=x_in, winners=winners)
    total = sum((val[head] * dz.detach().cpu().to(dtype)).sum() for (head, _), dz in zip(m.head_layers(), dzs))
    total.backward()
    return {i: W.grad.numpy().astype(np.float64) for i, W in leaves.items()}, pres


# ---------------------------------------------------------------------------------------------- the gate of the end-to-end tests
def forward_error(m, L, x, precision):
    """The forward's own error of the BatchNorm conv of layer row ``L`` on the float64 input ``x``, per output element: (K1 + 2) u x mass
    at fp32 and GATES[precision] x mass otherwise, mass = sum |w s| |x| + |bias| with the eval BatchNorm folded into s and the bias."""
    conv, bn = _conv_of(m, L.index), _bn_of(m, L.index)
    gamma, beta, mean, var = (_t64(v) for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s = (gamma / torch.sqrt(var + 1e-5))
    mass = fn.conv2d(x.abs(), (_t64(conv.weight) * s[:, None, None, None]).abs(), stride=L.stride, padding=L.size // 2).numpy() + \
        np.abs((beta - mean * s).numpy())[None, :, None, None]
    return ((conv.in_channels * L.size * L.size + 2) * U if GATES[precision] is None else GATES[precision]) * mass


def over_the_floor(label, m, layers, convs, precision, B, grads, want, floor, pres):
    """Per conv of ``convs``: asserts the mask-flip rule — a flip of the device's mask against the float64 pre-activation ``pres[c][0]``
    is legitimate only where |pre_64| is within the forward's own error (forward_error) — prints rms and max of
    (dW_dev - dW_64) / max |dW_64| beside the same figures of the float32 floor, and returns the [(conv, rms ratio, max ratio)] that
    exceed 4 x the floor (the caller asserts it empty after every figure is printed)."""
    over = []
    for c in convs:
        L = layers[c]
        pre, x = (a.detach() for a in pres[c])
        gate = forward_error(m, L, x, precision)
        y_dev = m.read_layer(c, B).cpu().numpy()
        flips = (pre.numpy() > 0) != (y_dev > 0)
        assert (np.abs(pre.numpy())[flips] <= gate[flips]).all(), (label, c, int(flips.sum()))
        got, ref = grads[c].cpu().numpy().astype(np.float64), np.abs(want[c]).max()
        assert got.shape == want[c].shape and ref > 0
        e_dev, e_32 = (got - want[c]) / ref, (floor[c] - want[c]) / ref
        rms = lambda e: float(np.sqrt(np.mean(e * e)))
        print("%s conv %d (stride %d, %d flips): rms %.3g (float32 floor %.3g, ratio %.2f)  max %.3g (floor %.3g, ratio %.2f)" % (
            label, c, L.stride, int(flips.sum()), rms(e_dev), rms(e_32), rms(e_dev) / rms(e_32), np.abs(e_dev).max(), np.abs(e_32).max(),
            np.abs(e_dev).max() / np.abs(e_32).max()))
        if not (rms(e_dev) <= 4 * rms(e_32) and np.abs(e_dev).max() <= 4 * np.abs(e_32).max()):
            over.append((c, round(rms(e_dev) / rms(e_32), 2), round(float(np.abs(e_dev).max() / np.abs(e_32).max()), 2)))
    return over


# ---------------------------------------------------------------------------------------------- the directional derivative
def cpu_scope_loss(m, t, B, images, grads, scope, x_in=None):
    """``cpu(s, dtype)``: the loss of the CPU model of the scope's sub-graph (torch's own leaky_relu and pools) at weights W + s g, on
    the device's boundary inputs (and ``x_in``, the prepared network input, where layer 0 is a member)."""
    W0 = {c: _conv_of(m, c).weight.detach().clone() for c in grads}
    heads = [h for h, _ in m.head_layers()]

    def cpu(s, dtype):
        with torch.no_grad():
            val, _, _ = cpu_graph(m, t, B, dtype, weights={c: W0[c].double() + s * grads[c].cpu().double() for c in grads}, scope=scope, x_in=x_in)
        acts = [val[h - 1].detach().numpy() for h in heads]
        ws = [_t64(_conv_of(m, h).weight).numpy() for h in heads]
        bs = [_t64(_conv_of(m, h).bias).numpy() for h in heads]
        if dtype != torch.float64:
            ws, bs = [a.astype(F) for a in ws], [a.astype(F) for a in bs]
        return cpu_head_model(acts, ws, bs, t.heads, images, 4, None if dtype == torch.float64 else dtype)["loss"]
    return cpu


def check_directional_derivative(m, t, xd, bnd, grads, cpu, l0):
    """The central difference of the device loss along -g, the convs of ``grads`` moved together by update_conv_weight, against ||g||^2.
    eps and the allowed gap come from the CPU model ``cpu(s, dtype)`` of the loss at weights W + s g, never from a device result: eps is
    the smallest of 1e-2, 3e-3, ... at which the modelled truncation gap still exceeds the float32 evaluation noise tenfold, and the
    check allows 4 * |fd_cpu - dd_cpu| + 2 * noise / (2 eps), dd_cpu the model's central difference at a tenth of eps, noise the
    largest float32 - float64 difference of the model at the three points 0, +eps, -eps."""
    g2 = sum(float((dw.double() ** 2).sum()) for dw in grads.values())
    masters = {c: _conv_of(m, c).weight.detach().clone().cuda() for c in grads}
    noise_at = lambda s: abs(cpu(s, torch.float32) - cpu(s, torch.float64))
    noise = noise_at(0.0)
    eps = gap_cpu = None
    for e in (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7):
        fd, dd = (cpu(e, torch.float64) - cpu(-e, torch.float64)) / (2 * e), (cpu(e / 10, torch.float64) - cpu(-e / 10, torch.float64)) / (2 * e / 10)
        if abs(fd - dd) >= 10 * noise / e:
            eps, gap_cpu = e, abs(fd - dd)
    assert eps is not None
    noise = max(noise, noise_at(eps), noise_at(-eps))                 # the largest of the three evaluations the quotient and the base use
    allowed = 4 * gap_cpu + 2 * noise / (2 * eps)

    def loss_at(s):
        for c in grads:
            m.update_conv_weight(c, masters[c] + s * grads[c])
        t.forward_loss(xd, bnd)
        return float(t.last_components[0].item())
    fd_dev = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
    assert loss_at(0.0) == l0                                         # the weights are back, bit for bit
    print("||g||^2 device %.8g; eps %.0e; central difference device %.8g; gap %.4g, allowed %.4g (cpu gap %.4g, noise %.4g)" % (g2, eps, fd_dev, abs(fd_dev - g2), allowed, gap_cpu, noise))
    assert g2 > 0 and abs(fd_dev - g2) <= allowed


# ---------------------------------------------------------------------------------------------- the training step
def check_training_steps(m, t, xd, bnd, scope, layers, trained, synced):
    """feed_forward_through_model, an SGD step and then two Adam steps (lr 1e-4): after each, the masters and moments of ``layers`` (the
    heads and the ``trained`` convs) equal block_grad_cases.opt_update_f32 of the gradients the scope's entry returned for the state
    before the step, and the packed image, as uint32 words, equals the host pack of the synchronised parameters (the ``synced`` convs'
    conv.weight then equal their masters).  Returns the losses."""
    from block_grad_cases import opt_update_f32
    losses = []
    host = lambda a: None if a is None else a.detach().cpu().numpy()
    for step, kind in enumerate(["sgd", "adam", "adam"]):
        if step < 2:
            t.optimizer = T.HeadOptimizer(kind, lr=1e-4)
        _, hg, ng = getattr(t, ENTRY[scope])(xd, bnd)
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
                    assert which == 1 and "bias" not in st and k in trained
                    continue
                zero = np.zeros_like(before[k][which])
                w1, m1, v1 = opt_update_f32(kind, before[k][which], grads[k][which], state[k].get("exp_avg" + sfx, zero), state[k].get("exp_avg_sq" + sfx, zero),
                                            1e-4, step=st["step"])
                assert np.array_equal(bits(host(st[name])), bits(w1)), (step, k, name)
                if kind == "adam":
                    assert np.array_equal(bits(host(st["exp_avg" + sfx])), bits(m1)) and np.array_equal(bits(host(st["exp_avg_sq" + sfx])), bits(v1)), (step, k, name)
        image = m.packed_weights()
        stream = m.weight_stream().copy()                             # synchronises the masters into the module's parameters
        assert all(_same(_conv_of(m, c).weight, t._head_masters[c][0]) for c in synced) and np.array_equal(image, pack(m._plan, stream)), step
    assert losses[1] != losses[0] and np.isfinite(losses).all(), losses
    return losses
