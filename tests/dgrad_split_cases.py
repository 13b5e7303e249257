"""What the host and GPU tests of the split-f16 data gradient (rtod_conv_dgrad_split, csrc/dgrad_split.hip) share: the inputs, a
float64 model of the entry's defined arithmetic, float32 references from the same operands, and the gate.

The model states what the FORMAT defines, free of any summation order (as tests/f16s3_emulation.py does for the forward):

* dz: per image b, a_b = max |dz[b]|, e_b = 13 - frexp(a_b).exp (a_b 2^e_b in [2^12, 2^13); a_b == 0: e_b = 0; held to -126 .. 126),
  v = dz 2^e_b (exact), hi = RNE_f16(v), lo = RNE_f16(v - hi);
* weights: v = float32(float64(w) * row_scale[o]) (w without a scale); row c of the gradient conv (the forward's input channel)
  is pre-scaled by 2^e_c with the rule of the forward's packed weights (channel_prescale, csrc/plan_weights.cpp): the maximum over o
  and taps of |float64(w) * row_scale| placed in [2^12, 2^13), e_c in -24 .. 40, an all-zero row e_c = 0; hi / lo by the same split;
* sum: hi*hi + hi*lo + lo*hi, evaluated as three float64 transposed convolutions (products of two halves are exact in float64);
  lo*lo is absent by definition;
* finish: dx = m(y) * (sum 2^-e_c 2^-e_b), m = 1 where y > 0 else float32(slope).

``model(..., mutant=name)`` plants one defect (MUTANTS); tests/test_dgrad_split_host.py requires the gate to catch each on every
case it applies to.  D = conv_T(|dz|, |v|) in float64 is the unit of every distance, r = (value - model) / D."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from f16s3_emulation import GATE_M, gate, rms_max  # noqa: F401  (re-exported: the tests take them from here)

# the issue's list for the CPU check: (B, Cout, Cin, H, W, size)
HOST_CASES = [(2, 512, 64, 13, 13, 3), (2, 1024, 512, 13, 13, 3), (2, 64, 32, 13, 13, 3), (2, 128, 64, 8, 104, 3), (2, 255, 64, 13, 13, 1)]
HOST_IMAGE_RATIO = 1000.0          # the two images of a batch, in magnitude
# the GPU cases: A band, one K group (M = 338 leaves a tail in every tile); B band, two K groups; C wide tile; D generic only; E slab;
# F ragged K; G generic 1x1
GPU_CASES = {"A": (2, 64, 32, 13, 13, 3), "B": (1, 512, 64, 13, 13, 3), "C": (1, 64, 128, 4, 104, 3), "D": (1, 32, 32, 3, 168, 3),
             "E": (2, 64, 32, 13, 13, 1), "F": (2, 255, 64, 13, 13, 1), "G": (2, 32, 32, 5, 7, 1)}
GPU_IMAGE_RATIO = 2.0 ** 10
SLOPE = float(np.float32(0.1))

# taps_not_flipped: the weights packed without the flip (size 3 only: a 1x1 conv has nothing to flip)
# hilo_dropped:     the hi*lo product (dz hi, weight lo) left out
# tensor_scale:     one power-of-two scale for the whole dz tensor instead of one per image
# ragged_k_chunk:   the last 32-wide K chunk of a cout that is no multiple of 32 left out (such couts only)
# mask_before_scale: the mask looked up before the image's scale is: m(y) of image 0 applied to every image.  (Merely swapping the
#                   two multiplications is the identity in exact arithmetic — both scales are powers of two — and no gate can see it;
#                   this is the defect that order invites: the mask indexed without the image.)  Batches of two or more only
MUTANTS = ("taps_not_flipped", "hilo_dropped", "tensor_scale", "ragged_k_chunk", "mask_before_scale")


def applicable(mutant, case):
    B, cout, cin, H, W, size = case
    if mutant == "taps_not_flipped":
        return size == 3
    if mutant == "ragged_k_chunk":
        return cout % 32 != 0
    if mutant in ("tensor_scale", "mask_before_scale"):
        return B >= 2
    return True


def make_inputs(case, ratio, seed=0, scaled=True):
    """-> (w float32 [Cout,Cin,k,k], row_scale float64 [Cout] or None, dz float32 [B,Cout,H,W], y float32 [B,Cin,H,W]).  dz is
    heavy-tailed (a normal times a log-normal of sigma 3: a few elements carry an image's maximum, most lie 2^-10 below it), image b
    is ``ratio ** -b`` of image 0; y has positives, negatives and exact zeros."""
    B, cout, cin, H, W, size = case
    g = torch.Generator().manual_seed(1000 * seed + cout + 7 * cin + H * W + size)
    w = (torch.randn(cout, cin, size, size, generator=g) / math.sqrt(cin * size * size)).float()
    scale = (torch.rand(cout, generator=g, dtype=torch.float64) * 2.8 + 0.2) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1) if scaled else None
    dz = torch.randn(B, cout, H, W, generator=g) * torch.exp(3.0 * torch.randn(B, cout, H, W, generator=g))
    dz = (dz * (float(ratio) ** -torch.arange(B, dtype=torch.float32)).view(B, 1, 1, 1) * 1e-3).float()
    y = torch.randn(B, cin, H, W, generator=g).float()
    y[torch.rand(B, cin, H, W, generator=g) < 0.1] = 0.0
    return w, scale, dz, y


def _split(v32):
    """hi, lo (float64) of a float32 tensor: RNE halves, subnormal halves included, no clamp (|v| < 2^13 here)."""
    hi = v32.half().float()
    lo = (v32 - hi).half().float()
    return hi.double(), lo.double()


def _exponent(a, lo_e, hi_e):
    e = 0
    if a > 0.0 and math.isfinite(a):
        e = 13 - math.frexp(a)[1]
    return max(lo_e, min(hi_e, e))


def folded(w, scale):
    """(v64 unrounded, v32 the float32 folded weight)."""
    v64 = w.double() if scale is None else w.double() * scale.view(-1, 1, 1, 1)
    return v64, v64.float()


def operands(w, scale, dz, tensor_scale=False):
    """The split operands in REAL units (float64): dz hi / lo [B,Cout,H,W], weight hi / lo [Cout,Cin,k,k], and the exponents."""
    v64, v32 = folded(w, scale)
    B, cin = dz.size(0), w.size(1)
    eb = [_exponent(float(dz.abs().max() if tensor_scale else dz[b].abs().max()), -126, 126) for b in range(B)]
    up = torch.tensor([2.0 ** e for e in eb], dtype=torch.float64).view(B, 1, 1, 1)
    zh, zl = _split((dz.double() * up).float())
    ec = [_exponent(float(v64[:, c].abs().max()), -24, 40) for c in range(cin)]
    ps = torch.tensor([2.0 ** e for e in ec], dtype=torch.float64).view(1, cin, 1, 1)
    wh, wl = _split((v32.double() * ps).float())
    return {"zh": zh / up, "zl": zl / up, "wh": wh / ps, "wl": wl / ps, "eb": eb, "ec": ec, "v32": v32, "zh_s": zh, "zl_s": zl, "wh_s": wh, "wl_s": wl,
            "up": up, "ps": ps}


def conv_t(a, w, size):
    return F.conv_transpose2d(a, w, None, 1, size // 2)


def mask_of(y, slope=SLOPE):
    if y is None or slope == 1.0:
        return None
    return torch.where(y > 0, torch.ones((), dtype=torch.float64), torch.full((), float(np.float32(slope)), dtype=torch.float64))


def model(w, scale, dz, y, size, slope=SLOPE, mutant=None):
    """The float64 model of rtod_conv_dgrad_split (optionally with one planted defect)."""
    op = operands(w, scale, dz, tensor_scale=mutant == "tensor_scale")
    zh, zl, wh, wl = op["zh"], op["zl"], op["wh"], op["wl"]
    if mutant == "taps_not_flipped":
        wh, wl = wh.flip(2, 3), wl.flip(2, 3)
    if mutant == "ragged_k_chunk":
        keep = (w.size(0) // 32) * 32
        zh, zl, wh, wl = zh[:, :keep], zl[:, :keep], wh[:keep], wl[:keep]
    acc = conv_t(zh, wh, size) + conv_t(zl, wh, size)
    if mutant != "hilo_dropped":
        acc = acc + conv_t(zh, wl, size)
    m = mask_of(y, slope)
    if m is None:
        return acc
    if mutant == "mask_before_scale":
        m = m[:1].expand_as(m)
    return m * acc


def truth(w, scale, dz, y, size, slope=SLOPE):
    """The exact float64 transposed conv of the same operands (dz, the float32 folded weight): what the format approximates."""
    acc = conv_t(dz.double(), folded(w, scale)[1].double(), size)
    m = mask_of(y, slope)
    return acc if m is None else m * acc


def unit(w, scale, dz, size):
    """D = conv_T(|dz|, |v|), float64; zeros (a pixel whose whole receptive field is zero) become 1 so that r is 0 there."""
    D = conv_t(dz.double().abs(), folded(w, scale)[1].double().abs(), size)
    return torch.where(D > 0, D, torch.ones_like(D))


def chunked_f32(op, size):
    """float32 accumulation of the three products in 32-wide K chunks in the kernels' K order (filter chunk outer, tap' inner), on
    the scaled planes as the MFMA sees them; each chunk's partial sum is torch's.  -> the raw sums times the exact inverse scales."""
    zh, zl, wh, wl = (op[k].float() for k in ("zh_s", "zl_s", "wh_s", "wl_s"))
    cout, pad = wh.size(0), size // 2
    zh, zl = (F.pad(t, (pad, pad, pad, pad)) for t in (zh, zl))
    H, W = zh.size(2) - 2 * pad, zh.size(3) - 2 * pad
    total = None
    for o0 in range(0, cout, 32):
        cs = slice(o0, min(cout, o0 + 32))
        for ky in range(size):                                    # tap' = (ky, kx) of the gradient conv reads the forward's tap (k-1-ky, k-1-kx)
            for kx in range(size):
                fy, fx = size - 1 - ky, size - 1 - kx
                kh, kl = (t[cs, :, fy, fx].t().contiguous().view(-1, cs.stop - cs.start, 1, 1) for t in (wh, wl))
                ah, al = zh[:, cs, ky:ky + H, kx:kx + W], zl[:, cs, ky:ky + H, kx:kx + W]
                t = (F.conv2d(ah, kh) + F.conv2d(ah, kl)) + F.conv2d(al, kh)
                total = t if total is None else total + t
    return total.double() / op["ps"] / op["up"]


def references(w, scale, dz, y, size, slope=SLOPE):
    """float32 evaluations of the same gradient from the same operands, each followed by the float32 mask multiplication: torch's
    conv_transpose2d on NCHW and on channels_last (dz, the float32 folded weight), and the chunked sum of the three products."""
    v32 = folded(w, scale)[1]
    m = mask_of(y, slope)
    m32 = None if m is None else m.float()
    fin = lambda t: (t if m32 is None else t.float() * m32).double()
    refs = {"nchw": fin(conv_t(dz, v32, size)),
            "channels_last": fin(conv_t(dz.contiguous(memory_format=torch.channels_last), v32.contiguous(memory_format=torch.channels_last), size).contiguous()),
            "chunked": fin(chunked_f32(operands(w, scale, dz), size).float())}
    return refs


def record(w, scale, dz, y, size, slope=SLOPE):
    """{"model", "D", "refs", "truth"}: what the gate needs (computed once per case and shared)."""
    return {"model": model(w, scale, dz, y, size, slope), "D": unit(w, scale, dz, size), "refs": references(w, scale, dz, y, size, slope),
            "truth": truth(w, scale, dz, y, size, slope)}


def residual(value, rec, against="model"):
    v = value.double() if isinstance(value, torch.Tensor) else torch.from_numpy(np.asarray(value, dtype=np.float64))
    return ((v - rec[against]) / rec["D"]).numpy()


def floors(rec, against="model", names=None):
    """(F_rms, F_max): the largest rms and the largest max of r over the float32 references (``names``: a subset of them)."""
    d = [rms_max(residual(v, rec, against)) for k, v in rec["refs"].items() if names is None or k in names]
    return max(a for a, _ in d), max(b for _, b in d)
