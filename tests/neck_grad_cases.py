"""What tests/test_neck_grad_host.py and tests/test_neck_grad_gpu.py share: rtod_plan_neck_layers on the C ABI, the neck convs the issue
expects per cfg, the shapes of the data-gradient and upsample-gradient tests, and exact references of rtod_conv_dgrad."""
import numpy as np

from scope_grad_cases import plan_list

F = np.float32
U = 2.0 ** -24

# the neck convs on fp32 plans: YOLOv3 layers 75-105 without the heads, routes and upsamples; YOLOv3-tiny (layer 8 is out: max-pool 9
# reads it); mini_cfg's small neck with route(-4), the upsample and route(-1, 10)
NECK = {"yolov3": [75, 76, 77, 78, 79, 80, 84, 87, 88, 89, 90, 91, 92, 96, 99, 100, 101, 102, 103, 104],
        "tiny": [12, 13, 14, 18, 21], "mini": [12, 13, 17, 20, 21], "fallback": [], "v5": []}

# (B, Cout, Cin, H, W) of the rtod_conv_dgrad tests: one pixel (only the centre tap sees it); every tap partly outside; rows that
# straddle the 64-column tile edge; ragged K per tap with a Cin tail tile and tiles crossing image boundaries; a rectangle;
# one-pixel-wide rows; a single row crossing a tile
DGRAD_SHAPES = [(1, 1, 32, 1, 1), (2, 18, 32, 2, 2), (1, 64, 64, 5, 7), (3, 255, 96, 13, 13), (2, 40, 32, 4, 6), (1, 64, 64, 127, 1), (1, 64, 64, 1, 70)]

# (H, W) of the input maps of the rtod_upsample2x_grad tests: everything clamped, one row, two rows, odd sizes, YOLOv3's 13 x 13
UPSAMPLE_SHAPES = [(1, 1), (1, 3), (2, 3), (5, 7), (13, 13)]


def neck_layers(h):
    return plan_list("rtod_plan_neck_layers", h, 2)


def conv_dgrad_ref(v, dz, dtype):
    """sum_{ky,kx,o} v[o,c,ky,kx] * dz[b,o,y+pad-ky,x+pad-kx] in ``dtype`` (np.int64 or np.float64), before the mask; dz outside the map 0."""
    cout, cin, size, _ = v.shape
    B, _, H, W = dz.shape
    pad = size // 2
    zp = np.zeros((B, cout, H + 2 * pad, W + 2 * pad), dtype)
    zp[:, :, pad:pad + H, pad:pad + W] = dz
    v = v.astype(dtype)
    out = np.zeros((B, cin, H, W), dtype)
    for ky in range(size):
        for kx in range(size):                                        # the window at (2 pad - ky, 2 pad - kx) of the padded map
            out += np.einsum("oc,bohw->bchw", v[:, :, ky, kx], zp[:, :, 2 * pad - ky:2 * pad - ky + H, 2 * pad - kx:2 * pad - kx + W])
    return out
