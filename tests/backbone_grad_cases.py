"""What tests/test_backbone_grad_host.py and tests/test_backbone_grad_gpu.py share: rtod_plan_trainable_layers on the C ABI, the trainable
convs expected per cfg, the shapes of the stride-2 kernel tests and exact numpy references of rtod_conv_dgrad_s2 / rtod_conv_wgrad_s2."""
import numpy as np

from scope_grad_cases import KEEP, plan_list

F = np.float32
U = 2.0 ** -24
BACKBONE = KEEP["backbone"]
UNFUSED = {"fuse_shortcut": 0, "fuse_pointwise": 0, "stem2_kernel": 0}

# with option keep_backbone_activations.  mini_cfg: every BatchNorm conv but layer 0; stride 2: 1, 5, 9, 10, 11; shortcuts 4 and 8;
# the route of layer 19 reaches back to layer 10.  YOLOv3-tiny: the neck (max-pools are not traversable)
TRAINABLE = {"mini": [1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 17, 20, 21], "tiny": [12, 13, 14, 18, 21]}
MINI_S2 = [1, 5, 9, 10, 11]

# (B, Cout, Cin, H, W), H x W the conv's INPUT map: only the centre tap; the smallest map with all four parity classes, one pixel each;
# odd size (the last odd row's tap looks outside the map); an odd rectangle; an even rectangle; ragged Cout, a Cin tail tile and classes
# crossing image boundaries; 72 pixels per class (each class crosses a 64-column tile edge); one pixel wide; one pixel high
S2_SHAPES = [(1, 1, 32, 1, 1), (1, 1, 32, 2, 2), (2, 18, 32, 3, 3), (1, 64, 64, 5, 7), (2, 40, 32, 4, 6), (3, 255, 96, 13, 13),
             (1, 64, 64, 16, 18), (1, 64, 64, 127, 1), (1, 64, 64, 1, 70)]


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def trainable_layers(h):
    return plan_list("rtod_plan_trainable_layers", h, 2)


def _tap_ranges(n_in, n_out, k):
    """The outputs o with 0 <= 2 o + k - 1 < n_in as a slice of the output axis, and the inputs 2 o + k - 1 they touch."""
    lo = 1 if k == 0 else 0
    hi = min(n_out - 1, (n_in - k) // 2)
    return slice(lo, hi + 1), slice(2 * lo + k - 1, 2 * hi + k, 2)


def conv_dgrad_s2_ref(v, dz, H, W, dtype):
    """dx[b,c,iy,ix] = sum over (ky,kx,o) with iy = 2 oy + ky - 1, ix = 2 ox + kx - 1 of v[o,c,ky,kx] * dz[b,o,oy,ox] in ``dtype``
    (np.int64 or np.float64), before the mask."""
    B, cout, Ho, Wo = dz.shape
    assert (Ho, Wo) == out_hw(H, W) and v.shape[2:] == (3, 3)
    v, dz = v.astype(dtype), dz.astype(dtype)
    out = np.zeros((B, v.shape[1], H, W), dtype)
    for ky in range(3):
        oy, iy = _tap_ranges(H, Ho, ky)
        for kx in range(3):
            ox, ix = _tap_ranges(W, Wo, kx)
            if oy.stop > oy.start and ox.stop > ox.start:
                out[:, :, iy, ix] += np.einsum("oc,bohw->bchw", v[:, :, ky, kx], dz[:, :, oy, ox])
    return out


def conv_wgrad_s2_ref(dz, x, dtype):
    """dW[o,c,ky,kx] = sum_{b,oy,ox} dz[b,o,oy,ox] * x[b,c,2 oy + ky - 1,2 ox + kx - 1] in ``dtype``, taps outside the map 0."""
    B, cout, Ho, Wo = dz.shape
    H, W = x.shape[2:]
    assert (Ho, Wo) == out_hw(H, W)
    dz, x = dz.astype(dtype), x.astype(dtype)
    out = np.zeros((cout, x.shape[1], 3, 3), dtype)
    for ky in range(3):
        oy, iy = _tap_ranges(H, Ho, ky)
        for kx in range(3):
            ox, ix = _tap_ranges(W, Wo, kx)
            if oy.stop > oy.start and ox.stop > ox.start:
                out[:, :, ky, kx] = np.einsum("bohw,bchw->oc", dz[:, :, oy, ox], x[:, :, iy, ix])
    return out


def taps_per_pixel(H, W):
    """The number of taps that reach input pixel (iy, ix): 1, 2, 2 or 4 by its parities."""
    return np.outer(1 + np.arange(H) % 2, 1 + np.arange(W) % 2)
