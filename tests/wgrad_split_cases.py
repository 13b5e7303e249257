"""What the host and GPU tests of the split-f16 weight gradient (rtod_conv_wgrad_split, csrc/wgrad_split.hip) share: the cases, the
inputs, a float64 model of the entry's defined arithmetic, float32 references from the same operands, and the gate.

The model states what the FORMAT defines, free of any summation order (as tests/dgrad_split_cases.py does for the data gradient):

* exponents: ONE per tensor (dW is a sum over the batch): a = max |t|, e = 13 - frexp(a).exp (a 2^e in [2^12, 2^13); a == 0 or not
  finite: e = 0; held to -126 .. 126); e_z for dz, e_x for x;
* split: v = t 2^e (exact), hi = RNE_f16(v), lo = RNE_f16(v - hi), subnormal halves kept;
* sum: zh*xh + zh*xl + zl*xh over all (b, y, x), each product one float64 torch.nn.grad.conv2d_weight on the scaled planes (products
  of two halves are exact in float64); zl*xl is absent by definition;
* finish: dW = float32(sum * 2^-(e_z + e_x) * row_scale[o]) (no scale: the factor 1).

``model(..., mutant=name)`` plants one defect (MUTANTS); tests/test_wgrad_split_host.py requires the gate to catch each on every case
it applies to.  D = |row_scale| * conv2d_weight(|x|, |dz|) in float64 is the unit of every distance, r = (value - model) / D."""
import math

import numpy as np
import torch

from f16s3_emulation import GATE_M, gate, rms_max  # noqa: F401  (re-exported: the tests take them from here)

# (B, Cout, Cin, H, W, size): the smallest shapes at which the kernel can still go wrong.  A odd width, pitch 16; B a map smaller than a
# k step's row group; C W % 8 == 0 and a Cout that leaves a tile tail; D ragged Cout and K = 507 (K % 8 != 0), 1x1; E a Cin that leaves
# a column tail, several tiles; F one row: six of nine taps see only padding; G K = 2704: several slices
CASES = {"A": (2, 64, 32, 13, 13, 3), "B": (1, 32, 64, 5, 7, 3), "C": (2, 96, 32, 4, 104, 3), "D": (3, 255, 64, 13, 13, 1),
         "E": (2, 32, 160, 26, 26, 3), "F": (2, 32, 32, 1, 9, 3), "G": (1, 64, 32, 52, 52, 3)}
IMAGE_RATIO = 2.0 ** 10            # the images of a batch, in magnitude
F_PADDING_ZEROS = 6144             # case F: elements of dW whose every term is padding (32 x 32 x the six taps of rows ky = 0, 2)

# x_lo_dropped:    the zh*xl product left out
# dz_lo_dropped:   the zl*xh product left out
# taps_flipped:    dW stored with the taps reversed (size 3 only)
# row_wraps:       tap kx reads across the end of a row into the next row, or image, instead of a zero: the defect a flat k grid without
#                  column halo invites (size 3 only)
# k_tail_dropped:  the last K % 8 pixels of the flat sum left out (size 1 with K % 8 != 0 only)
# image_exponent:  dz split with an exponent per image, but the tensor's one inverse applied (batches of two or more only)
MUTANTS = ("x_lo_dropped", "dz_lo_dropped", "taps_flipped", "row_wraps", "k_tail_dropped", "image_exponent")


def applicable(mutant, case):
    B, cout, cin, H, W, size = case
    if mutant in ("taps_flipped", "row_wraps"):
        return size == 3
    if mutant == "k_tail_dropped":
        return size == 1 and (B * H * W) % 8 != 0
    if mutant == "image_exponent":
        return B >= 2
    return True


def make_inputs(case, ratio=IMAGE_RATIO, seed=1, scaled=True):
    """-> (dz float32 [B,Cout,H,W], x float32 [B,Cin,H,W], row_scale float64 [Cout] or None).  dz is heavy-tailed (a normal times a
    log-normal of sigma 3) times 1e-3, image b ``ratio ** -b`` of image 0; x is leaky-shaped: a normal times a log-normal of sigma 1,
    negatives times 0.1, 10 % exact zeros; the scale lies in +-[0.2, 3]."""
    B, cout, cin, H, W, size = case
    g = torch.Generator().manual_seed(1000 * seed + cout + 7 * cin + H * W + size)
    dz = torch.randn(B, cout, H, W, generator=g) * torch.exp(3.0 * torch.randn(B, cout, H, W, generator=g))
    dz = (dz * (float(ratio) ** -torch.arange(B, dtype=torch.float32)).view(B, 1, 1, 1) * 1e-3).float()
    x = torch.randn(B, cin, H, W, generator=g) * torch.exp(1.0 * torch.randn(B, cin, H, W, generator=g))
    x = torch.where(x > 0, x, 0.1 * x).float()
    x[torch.rand(B, cin, H, W, generator=g) < 0.1] = 0.0
    scale = (torch.rand(cout, generator=g, dtype=torch.float64) * 2.8 + 0.2) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    return dz, x, (scale if scaled else None)


def exponent(a):
    e = 0
    if a > 0.0 and math.isfinite(a):
        e = 13 - math.frexp(a)[1]
    return max(-126, min(126, e))


def _split(v32):
    """hi, lo (float64) of a float32 tensor: RNE halves, subnormal halves included (|v| < 2^13 here)."""
    hi = v32.half().float()
    lo = (v32 - hi).half().float()
    return hi.double(), lo.double()


def wg(x, dz, size):
    """dW[o][c][ky][kx] = sum dz[b,o,y,x] x[b,c,y+ky-p,x+kx-p] in the dtype of the operands."""
    return torch.nn.grad.conv2d_weight(x, (dz.size(1), x.size(1), size, size), dz, stride=1, padding=size // 2)


def operands(dz, x, image_exponent=False):
    """The scaled split planes (float64) and the two exponents."""
    ez, ex = exponent(float(dz.abs().max())), exponent(float(x.abs().max()))
    B = dz.size(0)
    eb = [exponent(float(dz[b].abs().max())) if image_exponent else ez for b in range(B)]
    up = torch.tensor([2.0 ** e for e in eb], dtype=torch.float64).view(B, 1, 1, 1)
    zh, zl = _split((dz.double() * up).float())
    xh, xl = _split((x.double() * 2.0 ** ex).float())
    return {"zh": zh, "zl": zl, "xh": xh, "xl": xl, "ez": ez, "ex": ex}


def _col(scale, cout):
    return torch.ones(cout, 1, 1, 1, dtype=torch.float64) if scale is None else scale.double().view(-1, 1, 1, 1)


def _finish(acc, op, scale):
    """One multiplication in double, one rounding to float32 (returned as float64)."""
    return (acc.double() * 2.0 ** -(op["ez"] + op["ex"]) * _col(scale, acc.size(0))).float().double()


def _wrapped(t, kx):
    """x as tap column kx of a flat [B * H * W] grid without column halo sees it: position x + kx - 1 taken from the flat index, so
    the end of a row continues in the next row or image; zeros outside the whole array alone.  Returned already shifted: column x
    holds what the tap reads there."""
    B, C, H, W = t.shape
    flat = t.permute(1, 0, 2, 3).reshape(C, -1)
    s = torch.zeros_like(flat)
    if kx == 0:
        s[:, 1:] = flat[:, :-1]
    elif kx == 2:
        s[:, :-1] = flat[:, 1:]
    else:
        s = flat
    return s.view(C, B, H, W).permute(1, 0, 2, 3).contiguous()


def _product(zp, xp, size, mutant):
    if mutant == "row_wraps":                                         # the column shift done on the flat grid, the row taps as they should be
        cols = [torch.nn.grad.conv2d_weight(_wrapped(xp, kx), (zp.size(1), xp.size(1), 3, 1), zp, stride=1, padding=(1, 0)) for kx in range(3)]
        return torch.cat(cols, dim=3)
    if mutant == "k_tail_dropped":
        B, _, H, W = zp.shape
        keep = torch.ones(B * H * W, dtype=zp.dtype)
        keep[B * H * W - (B * H * W) % 8:] = 0.0
        zp = zp * keep.view(B, 1, H, W)
    return wg(xp, zp, size)


def model(dz, x, scale, size, mutant=None):
    """The float64 model of rtod_conv_wgrad_split (optionally with one planted defect)."""
    op = operands(dz, x, image_exponent=mutant == "image_exponent")
    acc = _product(op["zh"], op["xh"], size, mutant)
    if mutant != "x_lo_dropped":
        acc = acc + _product(op["zh"], op["xl"], size, mutant)
    if mutant != "dz_lo_dropped":
        acc = acc + _product(op["zl"], op["xh"], size, mutant)
    if mutant == "taps_flipped":
        acc = acc.flip(2, 3)
    return _finish(acc, op, scale)


def truth(dz, x, scale, size):
    """The exact float64 weight gradient of the same operands: what the format approximates."""
    return wg(x.double(), dz.double(), size) * _col(scale, dz.size(1))


def unit_raw(dz, x, scale, size):
    return wg(x.double().abs(), dz.double().abs(), size) * _col(scale, dz.size(1)).abs()


def references(dz, x, scale, size):
    """float32 evaluations of the same gradient from the same operands, each finished by the same double multiplication and rounding:
    torch's conv2d_weight on NCHW and on channels_last, and the three products accumulated in float32 on the scaled planes."""
    op = operands(dz, x)
    col = _col(scale, dz.size(1))
    fin = lambda t: (t.double() * col).float().double()
    cl = torch.channels_last
    zh, zl, xh, xl = (op[k].float() for k in ("zh", "zl", "xh", "xl"))
    return {"nchw": fin(wg(x, dz, size)),
            "channels_last": fin(wg(x.contiguous(memory_format=cl), dz.contiguous(memory_format=cl), size).contiguous()),
            "f32x3": _finish((wg(xh, zh, size) + wg(xl, zh, size)) + wg(xh, zl, size), op, scale)}


def record(dz, x, scale, size):
    """{"model", "D", "zero", "refs", "truth"}: what the gate needs (computed once per case and shared).  "zero": the elements of dW whose
    every term is zero (D == 0 before the zeros become 1)."""
    raw = unit_raw(dz, x, scale, size)
    return {"model": model(dz, x, scale, size), "D": torch.where(raw > 0, raw, torch.ones_like(raw)), "zero": raw == 0,
            "refs": references(dz, x, scale, size), "truth": truth(dz, x, scale, size)}


def residual(value, rec, against="model"):
    v = value.double() if isinstance(value, torch.Tensor) else torch.from_numpy(np.asarray(value, dtype=np.float64))
    return ((v - rec[against]) / rec["D"]).numpy()


def floors(rec, against="model", names=None):
    """(F_rms, F_max): the largest rms and the largest max of r over the float32 references (``names``: a subset of them)."""
    d = [rms_max(residual(v, rec, against)) for k, v in rec["refs"].items() if names is None or k in names]
    return max(a for a, _ in d), max(b for _, b in d)
