"""What the host and GPU tests of the "full" training scope share (max-pool backward, thin-conv gradients, layer 0): the shapes of the
kernel tests, numpy references of the max-pool backward with the forward's first-maximum rule, the plan's listing entry, and the CPU
model of the full sub-graph — scope_grad_cases.cpu_graph with two more kinds: a [maxpool] written as a gather with the DEVICE's winners
(or torch's own pool), and layer 0 fed the prepared network input."""
import numpy as np
import torch

import scope_grad_cases as S
from head_grad_cases import cpu_head_model
from scope_grad_cases import _bn_of, _box, _conv_of, _t64, plan_list

F = np.float32
U = 2.0 ** -24
fn = torch.nn.functional
FULL = {"keep_head_inputs": 1, "keep_full_activations": 1}
S.KEEP.setdefault("full", FULL)                                       # scope_trainer / check_training_steps look their scope up
S.ENTRY.setdefault("full", "full_gradients")

# (B, C, H, W, stride) of rtod_maxpool_grad: one pixel, one window, odd last row / column, the clamped pool on odd maps, tiny's 13 x 13
# stride-1 pool, more than one block, one row (every window clamped in y), one column whose stride-2 output is empty
POOL_SHAPES = [(1, 1, 1, 1, 1), (1, 1, 2, 2, 2), (1, 3, 5, 7, 2), (2, 5, 5, 7, 1), (1, 16, 13, 13, 1), (2, 32, 26, 26, 2), (1, 1, 1, 70, 1), (1, 1, 127, 1, 2)]
# (B, Cout, Cin, H, W, size) of rtod_conv_wgrad_thin; the last: K = 8190 spans 32 slices of 256, the last one of 254 terms
WGRAD_THIN_SHAPES = [(1, 1, 1, 1, 1, 3), (1, 16, 3, 8, 8, 3), (2, 32, 16, 5, 7, 3), (1, 16, 3, 1, 70, 3), (3, 24, 16, 13, 13, 1), (1, 70, 5, 9, 9, 3),
                     (2, 16, 3, 63, 65, 3)]
DGRAD_THIN_SHAPES = [(1, 1, 1, 1, 1, 3), (2, 32, 16, 5, 7, 3), (1, 255, 16, 13, 13, 1), (1, 18, 3, 4, 6, 3), (1, 32, 16, 1, 70, 3)]
TINY_FULL = [0, 2, 4, 6, 8, 10, 12, 13, 14, 18, 21]
POOL_MINI_FULL = {16: [0, 2, 4, 6, 8, 9, 10, 14, 17], 32: [2, 4, 6, 8, 9, 10, 14, 17]}
POOL_MINI_TRAINABLE = [8, 9, 10, 14, 17]


def full_layers(h):
    return plan_list("rtod_plan_full_layers", h, 2)


def pool_out_hw(H, W, stride):
    return (H, W) if stride == 1 else (H // 2, W // 2)


# ---------------------------------------------------------------------------------------------- the max-pool and its backward
def pool_winners(x, stride):
    """Flat index (clamped y * W + clamped x) of the winner of every size-2 window of ``x`` [B,C,H,W]: scan dy then dx, the FIRST maximum
    wins (np.argmax over the taps in scan order).  Stride 2: floor mode; stride 1: the clamped window.  -> int64 [B,C,Ho,Wo]."""
    B, C_, H, W = x.shape
    Ho, Wo = pool_out_hw(H, W, stride)
    oy, ox = np.arange(Ho), np.arange(Wo)
    vals, flat = [], []
    for dy in range(2):
        yy = np.minimum(oy * stride + dy, H - 1)
        for dx in range(2):
            xx = np.minimum(ox * stride + dx, W - 1)
            vals.append(x[:, :, yy[:, None], xx[None, :]])
            flat.append(np.broadcast_to(yy[:, None] * W + xx[None, :], (B, C_, Ho, Wo)))
    k = np.argmax(np.stack(vals), axis=0)
    return np.take_along_axis(np.stack(flat), k[None], axis=0)[0].astype(np.int64)


def maxpool_grad_ref(dz, x, stride, dtype=np.float64):
    """``(dx, mass)`` in ``dtype``: dz of every window scattered onto its winner (pool_winners), before the mask, and the same sum of
    |dz| (the mass of the contributions an element received)."""
    B, C_, H, W = x.shape
    win = pool_winners(x, stride).reshape(B * C_, -1)
    out, mass = np.zeros((B * C_, H * W), dtype), np.zeros((B * C_, H * W), dtype)
    rows = np.repeat(np.arange(B * C_), win.shape[1])
    np.add.at(out, (rows, win.ravel()), dz.astype(dtype).ravel())
    np.add.at(mass, (rows, win.ravel()), np.abs(dz.astype(dtype)).ravel())
    return out.reshape(B, C_, H, W), mass.reshape(B, C_, H, W)


def torch_pool(x, stride):
    """The reference's two modules: nn.MaxPool2d(2, 2), and MaxPoolStride1 (replicate pad right / bottom, then MaxPool2d(2, 1))."""
    return fn.max_pool2d(x, 2, 2) if stride == 2 else fn.max_pool2d(fn.pad(x, (0, 1, 0, 1), mode="replicate"), 2, 1)


def torch_pool_grad(dz, x, stride):
    """CPU autograd of torch_pool in the dtype of ``x`` (numpy in, numpy out); an empty output map gives zeros."""
    if dz.size == 0:
        return np.zeros_like(x)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    torch_pool(xt, stride).backward(torch.from_numpy(dz.copy()))
    return xt.grad.numpy()


# ---------------------------------------------------------------------------------------------- the fixed batch at any size
def full_batch(height, width, classes, B=3):
    """scope_grad_cases.step_batch's boxes scaled to a ``height`` x ``width`` input (they are laid out on 64 x 64), ``classes`` classes."""
    s = min(height, width) / 64.0
    box = lambda cx, cy, w, h, cls=0: _box(cx * s, cy * s, w * s, h * s, classes, cls)
    return [np.stack([box(20, 22, 30, 26), box(45, 40, 24, 36), box(33, 50, 50, 18)]), np.zeros((0, 5 + classes), F),
            np.stack([box(10, 50, 12, 40), box(52, 12, 20, 20, cls=2), box(40, 30, 60, 60)])][:B]


# ---------------------------------------------------------------------------------------------- the CPU model of the full sub-graph
def cpu_full_graph(m, t, B, dtype, x_in, weights=None, masks=None, winners=None):
    """scope_grad_cases.cpu_graph for scope "full": ``x_in`` is the prepared network input (what layer 0 reads); a [maxpool] is a gather
    with ``winners[layer]`` (pool_winners of the DEVICE's read_layer copy of the pool's input) where given, else torch's own pool.
    Returns (values per layer, {conv: leaf weight}, {conv: (pre-activation, input)}, {pool: its input value})."""
    layers, readers, member, scales = t._graph("full")
    cast = lambda a: torch.as_tensor(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).to(dtype)
    val, leaves, pres, pooled = {-1: cast(x_in)}, {}, {}, {}

    def value(src):
        if src not in val:
            assert not member[src]
            val[src] = cast(m.read_layer(src, B))
        return val[src]

    for L in layers:
        i = L.index
        if not member[i]:
            continue
        if L.type == "convolutional":
            conv, x = _conv_of(m, i), value(i - 1)
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
            x = value(i - 1)
            pooled[i] = x
            if winners is None:
                val[i] = torch_pool(x, L.stride)
            else:
                idx = torch.from_numpy(winners[i])
                val[i] = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
        elif L.type == "upsample":
            x = value(i - 1)
            val[i] = fn.interpolate(x, scale_factor=2, mode="nearest") if L.nearest else fn.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        elif L.type == "shortcut":
            val[i] = value(L.srcs[0]) + value(L.srcs[1])
        else:
            parts, off = [], 0
            for s in L.srcs:
                parts.append(value(s) if member[s] else cast(m.read_layer(i, B))[:, off:off + layers[s].cout])
                off += layers[s].cout
            val[i] = torch.cat(parts, 1)
    return val, leaves, pres, pooled


def cpu_full_grads(m, t, B, dtype, x_in, masks, winners, dzs):
    val, leaves, pres, pooled = cpu_full_graph(m, t, B, dtype, x_in, masks=masks, winners=winners)
    total = sum((val[head] * dz.detach().cpu().to(dtype)).sum() for (head, _), dz in zip(m.head_layers(), dzs))
    total.backward()
    return {i: W.grad.numpy().astype(np.float64) for i, W in leaves.items()}, pres, pooled


def cpu_full_loss(m, t, B, images, grads, x_in):
    """scope_grad_cases.cpu_scope_loss over cpu_full_graph with torch's own leaky_relu and pools."""
    W0 = {c: _conv_of(m, c).weight.detach().clone() for c in grads}
    heads = [h for h, _ in m.head_layers()]

    def cpu(s, dtype):
        with torch.no_grad():
            val = cpu_full_graph(m, t, B, dtype, x_in, weights={c: W0[c].double() + s * grads[c].cpu().double() for c in grads})[0]
        acts = [val[h - 1].detach().numpy() for h in heads]
        ws = [_t64(_conv_of(m, h).weight).numpy() for h in heads]
        bs = [_t64(_conv_of(m, h).bias).numpy() for h in heads]
        if dtype != torch.float64:
            ws, bs = [a.astype(F) for a in ws], [a.astype(F) for a in bs]
        return cpu_head_model(acts, ws, bs, t.heads, images, 4, None if dtype == torch.float64 else dtype)["loss"]
    return cpu


def winner_flips_within_the_forward_error(label, m, layers, pool, winners, x64, precision, x_in):
    """The winner-flip rule, beside over_the_floor's mask-flip rule: where the device's winner of a window of ``pool`` is not the maximum
    of the float64 model's input ``x64`` [B,C,H,W], the two float64 values may differ by no more than the forward's own error at the conv
    that produced them — (K + 2) u x mass at fp32, GATES[precision] x mass otherwise, each of the two values with its own mass (their
    sum bounds the difference).  A pool that reads no conv of the graph admits no flip.  Returns the number of flips."""
    x = x64.detach().numpy()
    L = layers[pool]
    B, C_, H, W = x.shape
    flat = x.reshape(B, C_, -1)
    dev = np.take_along_axis(flat, winners.reshape(B, C_, -1), 2)
    best = torch_pool(torch.from_numpy(x), L.stride).numpy().reshape(B, C_, -1)
    flips = dev != best
    n = int(flips.sum())
    if n == 0:
        return 0
    src = pool - 1
    assert layers[src].type == "convolutional" and layers[src].bn, (label, pool, n)
    conv, bn, P = _conv_of(m, src), _bn_of(m, src), layers[src]
    gamma, beta, mean, var = (_t64(v) for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s = gamma / torch.sqrt(var + 1e-5)
    xin = _t64(m.read_layer(src - 1, B)) if src > 0 else _t64(x_in)
    mass = fn.conv2d(xin.abs(), (_t64(conv.weight) * s[:, None, None, None]).abs(), stride=P.stride, padding=P.size // 2).numpy() + \
        np.abs((beta - mean * s).numpy())[None, :, None, None]
    gate = ((conv.in_channels * P.size * P.size + 2) * U if S.GATES[precision] is None else S.GATES[precision]) * mass
    gate_dev = np.take_along_axis(gate.reshape(B, C_, -1), winners.reshape(B, C_, -1), 2)
    gate_best = torch_pool(torch.from_numpy(gate), L.stride).numpy().reshape(B, C_, -1)     # an upper bound of the true maximum's own gate
    assert (np.abs(dev - best)[flips] <= (gate_dev + gate_best)[flips]).all(), (label, pool, n)
    return n
