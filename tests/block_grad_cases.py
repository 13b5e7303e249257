"""What tests/test_block_grad_host.py and tests/test_block_grad_gpu.py share: the slice rule of rtod_conv_wgrad restated from
include/rtod.h, rtod_plan_head_blocks on the C ABI, exact references of the two gradient kernels, and the optimiser step of
rtod_plan_step_conv restated in float32 numpy (one rounding per documented line)."""
import numpy as np

from scope_grad_cases import plan_list

F = np.float32
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------- rtod_conv_wgrad's slice rule
def conv_wgrad_slices(K, cout, ncol):
    """include/rtod.h: tiles = ceil(cout / 64) * ceil(ncol / 64), ncol = cin * size * size; cap = min(16, ceil(1024 / tiles));
    units = ceil(K / 8); L = 8 * ceil(units / cap); S = ceil(K / L).  Returns (S, L, cap)."""
    tiles = ((cout + 63) // 64) * ((ncol + 63) // 64)
    cap = min(16, (1024 + tiles - 1) // tiles)
    units = (K + 7) // 8
    L = 8 * ((units + cap - 1) // cap)
    return (K + L - 1) // L, L, cap


# The shapes (B, Cout, Cin, H, W) of the GPU tests of rtod_conv_wgrad: one pixel (only the centre tap sees it); mini_cfg's grid; a
# rectangle; chunks that cross image boundaries with a Cout tail; a second rectangle; then shapes chosen from the slice rule (3x3):
# S = 1 with many tiles, S = 2 = the cap (524 tiles), S = 16 with K exactly on a slice boundary (128 = 16 * 8) and one short of it.
# tests/test_block_grad_host.py holds them to the library's own slice counts.
WGRAD_SHAPES = [(1, 1, 32, 1, 1), (2, 18, 32, 2, 2), (1, 64, 64, 5, 7), (3, 255, 96, 13, 13), (2, 40, 32, 4, 6),
                (1, 64, 512, 2, 4), (2, 256, 928, 4, 4), (1, 64, 64, 16, 8), (1, 64, 64, 127, 1)]


def head_blocks(h):
    return plan_list("rtod_plan_head_blocks", h, 3)


# ---------------------------------------------------------------------------------------------- references of the kernels
def wgrad_ref(dz, x, size, dtype):
    """dW[o,c,ky,kx] = sum_{b,y,x} dz[b,o,y,x] * x[b,c,y+ky-pad,x+kx-pad] in ``dtype`` (np.int64 or np.float64), taps outside the map 0."""
    B, cout, H, W = dz.shape
    pad = size // 2
    xp = np.zeros((B, x.shape[1], H + 2 * pad, W + 2 * pad), dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    dz = dz.astype(dtype)
    out = np.zeros((cout, x.shape[1], size, size), dtype)
    for ky in range(size):
        for kx in range(size):
            out[:, :, ky, kx] = np.einsum("bohw,bchw->oc", dz, xp[:, :, ky:ky + H, kx:kx + W])
    return out


def dgrad_ref(w, dz, dtype):
    """sum_o w[o,c] * dz[b,o,p] in ``dtype``, before the mask."""
    return np.einsum("oc,bop->bcp", w.astype(dtype), dz.astype(dtype))


# ---------------------------------------------------------------------------------------------- opt_update in float32, on the host
def _fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays with ONE rounding.  a * b is exact in float64 (48 bits); s = fl64(a * b + c) with its
    rounding error e from Knuth's two-sum.  Rounding s to float32 equals rounding the exact sum unless s is exactly halfway between
    two float32 values while e != 0: no float64 (and a float32 midpoint is one) lies strictly between the exact sum and its nearest
    float64.  There s is nudged one float64 ulp towards the exact sum first."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s32 = s.astype(F)
    lo, hi = np.nextafter(s32, F(-np.inf)).astype(np.float64), np.nextafter(s32, F(np.inf)).astype(np.float64)
    tie = (e != 0) & np.isfinite(s) & ((s == 0.5 * (lo + s32.astype(np.float64))) | (s == 0.5 * (hi + s32.astype(np.float64))))
    s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def opt_update_f32(kind, w, g, m, v, lr, betas=(0.9, 0.999), eps=1e-8, step=1):
    """One step as include/rtod.h documents it at rtod_plan_step_conv, float32 with one rounding per line; lr, betas and eps are the
    decimals the caller wrote (the library reads its float fields as their shortest decimals).  Returns (w', m', v')."""
    w, g = np.asarray(w, F), np.asarray(g, F)
    if kind == "sgd":
        return (w - (F(lr) * g).astype(F)).astype(F), m, v
    b1, b2 = betas
    a, r = F(lr / (1.0 - b1 ** step)), F(np.sqrt(1.0 - b2 ** step))
    c1, c2 = F(1.0 - b1), F(1.0 - b2)
    d = (g - m).astype(F)
    m1 = _fma32(d, np.full_like(d, c1), m)
    q = (g * g).astype(F)
    p = (F(b2) * v).astype(F)
    v1 = _fma32(q, np.full_like(q, c2), p)
    s = np.sqrt(v1).astype(F)
    s = (s / r).astype(F)
    den = (s + F(eps)).astype(F)
    u = (m1 / den).astype(F)
    return _fma32(np.full_like(u, -a), u, w), m1, v1
