"""What the host and GPU tests of the "full" training scope share (max-pool backward, thin-conv gradients, layer 0): the shapes of the
kernel tests, numpy references of the max-pool backward with the forward's first-maximum rule, the plan's listing entry, the fixed
batch at any size and the winner-flip rule.  The CPU model of the full sub-graph is scope_grad_cases.cpu_graph (its [maxpool] arm and
its network-input value)."""
import numpy as np
import torch

from scope_grad_cases import KEEP, _box, _t64, forward_error, plan_list, torch_pool

F = np.float32
U = 2.0 ** -24
FULL = KEEP["full"]

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


# ---------------------------------------------------------------------------------------------- the winner-flip rule
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
    gate = forward_error(m, layers[src], _t64(m.read_layer(src - 1, B)) if src > 0 else _t64(x_in), precision)
    gate_dev = np.take_along_axis(gate.reshape(B, C_, -1), winners.reshape(B, C_, -1), 2)
    gate_best = torch_pool(torch.from_numpy(gate), L.stride).numpy().reshape(B, C_, -1)     # an upper bound of the true maximum's own gate
    assert (np.abs(dev - best)[flips] <= (gate_dev + gate_best)[flips]).all(), (label, pool, n)
    return n
