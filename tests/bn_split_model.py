"""Square probes and the layer-local float64 model of batch-statistics BatchNorm on the split-f16 kernels (plan options
bn_batch_stats + bn_batch_split, precision 1).  Test helper of tests/test_bn_split_host.py and tests/test_bn_split_gpu.py.

bn_batch_stats is square-only, so the rectangular probes of conv_probes.PROBES do not apply; SQUARE lists square ones of the same
construction (conv_probes.Probe: stem, optional 1x1, the conv under test, optional shortcut, linear head + yolo).

The model of ONE BatchNorm conv layer, from its stored input ``a`` and stored shortcut operand ``res`` (float64; on the GPU: what
read_layer returns), states what the mode defines, free of any summation order:

* the conv is unfolded (plan.cpp load_weights under bn_batch_stats: scale 1, no bias).  After layer 0 its sum is the three
  products ah*wh + ah*wl + al*wh of the split planes of the input and of the pre-scaled weights (f16s3_emulation.folded_weights
  with scale 1), in float64.  Layer 0 runs the exact-fp32 kernel: the float64 convolution with the float32 weights;
* mean and biased variance per channel over (B, H, W), float64;
* w_c = gamma / sqrt(var + 1e-5), b_c = beta - mean w_c; y = act(raw w_c + b_c) + shortcut; the store split (store_split).

Unit of every distance: D = |w_c| conv(|a|, |w|) + |beta| + |shortcut|.  Floors: float32 evaluations of the same layer from the
same inputs (torch NCHW, channels_last, the kernels' chunked K order), each followed by double statistics of the float32 sums, a
float32 normalise with the kernels' per-channel constants and the float32 store split.  Gate: f16s3_emulation.gate (GATE_M = 4).

``mutant`` plants one defect in the model (MUTANTS); the host test requires the gate to catch each of them.
"""
import dataclasses
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_probes import Probe
from f16_emulation import _fused_away
from f16s3_emulation import LEAKY, SCALE, conv_chunked_f32, folded_weights, split_planes, store_split, store_split_f32

EPS = 1e-5
BN_OPTIONS = (("bn_batch_stats", 1), ("bn_batch_split", 1))
MUTANTS = ("stats_per_frame", "shortcut_lo", "const_neighbour")


def _p(name, shape, B, note, **kw):
    return Probe(name, *shape, B, note=note, **kw)


SQUARE = [
    _p("a_band96", (12, 12, 96, 96, 3, 1), 3, "bandd 61-63, 66; odd K chunks; Cout 96: one-stage statistics; 144 pixels per frame: a frame boundary and a ragged tail in every M tile", shortcut=True),
    _p("b_band_k2", (20, 20, 512, 64, 3, 1), 2, "H W = 400: the two-K-group bandd tiles 64, 65, 67, 69"),
    _p("c_band_k1", (21, 21, 512, 64, 3, 1), 2, "H W = 441: the one-group bandd tiles"),
    _p("d_wide", (96, 96, 32, 128, 3, 1), 2, "generic 0-11 and the wide bandd tile 68"),
    _p("e_slab192", (14, 14, 192, 96, 1, 1), 3, "1x1 slab tiles 90-100 and generic; Cout 96"),
    _p("f_slab64", (14, 14, 64, 32, 1, 1), 3, "one 64-channel slab, Cout below the tile width", options=(("fuse_pointwise", 0),)),
    _p("g_pw96", (14, 14, 96, 32, 1, 1), 3, "a 1x1 layer the slab family must refuse (Cin % 64 != 0): generic only"),
    _p("h_s2", (22, 22, 64, 96, 3, 2), 3, "stride 2 onto 11x11: generic"),
    _p("i_silu", (12, 12, 96, 96, 3, 1), 3, "shape of a, SiLU", act="silu", shortcut=True),
    _p("j_linear", (12, 12, 96, 96, 3, 1), 3, "shape of a, linear", act="linear", shortcut=True),
]
BY_NAME = {p.name: p for p in SQUARE}


def with_bn_options(p):
    """The probe with the mode's two options appended (bn_batch_stats first: it is set while the plan is still exact fp32)."""
    return dataclasses.replace(p, options=tuple(p.options) + BN_OPTIONS)


def _act(y, L):
    if L.leaky:
        return torch.where(y > 0, y, y * (LEAKY if y.dtype == torch.float64 else 0.1))
    if L.silu:
        return y * torch.sigmoid(y)
    return y


def _stats(raw, per_frame=False):
    """Per-channel mean and biased variance in float64 over (B, H, W); ``per_frame``: over (H, W) of every frame (a defect)."""
    r = raw.double()
    dims = (2, 3) if per_frame else (0, 2, 3)
    mean = r.mean(dims, keepdim=True)
    var = (r * r).mean(dims, keepdim=True) - mean * mean
    return mean, var.clamp(min=0)


def bn_layer_model(L, p, a, res, mutant=None, references=False):
    """Record of BatchNorm conv ``L`` (oracle IR layer, parameters ``p``) from stored input ``a`` and shortcut operand ``res``
    (float64, or None): {"model", "D", "refs", "mean", "var"} (f16s3_emulation.residual / floors / gate apply)."""
    assert L.bn
    a = a.double()
    res = None if res is None else res.double()
    w32 = p["weight"].float()
    conv = lambda x, w: F.conv2d(x, w, None, L.stride, L.pad)
    if L.index == 0:                                           # exact-fp32 kernel
        raw = conv(a, w32.double())
    else:
        W = folded_weights({"weight": p["weight"], "bias": torch.zeros(L.cout)}, SimpleNamespace(bn=False, cout=L.cout))
        hi, lo = split_planes(a * SCALE)
        ah, al = hi / SCALE, lo / SCALE
        raw = conv(ah, W["wh"]) + conv(ah, W["wl"]) + conv(al, W["wh"])
    gamma, beta = p["gamma"].double().view(1, -1, 1, 1), p["beta"].double().view(1, -1, 1, 1)
    mean, var = _stats(raw, per_frame=mutant == "stats_per_frame")
    wc = gamma / torch.sqrt(var + EPS)
    bc = beta - mean * wc
    if mutant == "const_neighbour":                            # the normalise constants of channel c + 1
        wc, bc = torch.roll(wc, -1, 1), torch.roll(bc, -1, 1)
    y = _act(raw * wc + bc, L)
    if res is not None:
        y = y + (split_planes(res * SCALE)[0] / SCALE if mutant == "shortcut_lo" else res)
    D = wc.abs() * conv(a.abs(), w32.double().abs()) + beta.abs()
    if res is not None:
        D = D + res.abs()
    rec = {"conv": L.index, "model": store_split(y), "D": D, "refs": {}, "mean": mean.flatten(), "var": var.flatten()}
    if references:
        a32 = a.float()
        r32 = None if res is None else res.float()
        g64, b64 = p["gamma"].double().view(1, -1, 1, 1), p["beta"].double().view(1, -1, 1, 1)

        def finish(raw32):
            raw32 = raw32.contiguous()
            m, v = _stats(raw32)                               # double statistics of the float32 sums
            invstd = 1.0 / torch.sqrt(v + EPS)
            w = (invstd * g64).float()                         # the kernels' per-channel constants (bn_apply_kernel)
            b = (b64 - m * invstd * g64).float()
            y32 = _act(raw32 * w + b, L)
            if r32 is not None:
                y32 = y32 + r32
            return store_split_f32(y32)

        rec["refs"]["nchw"] = finish(F.conv2d(a32, w32, None, L.stride, L.pad))
        rec["refs"]["channels_last"] = finish(F.conv2d(a32.contiguous(memory_format=torch.channels_last),
                                                       w32.contiguous(memory_format=torch.channels_last), None, L.stride, L.pad))
        rec["refs"]["chunked"] = finish(conv_chunked_f32(a32, w32, L))
    return rec


def bn_layers(ref):
    """[(conv layer, stored layer, input layer or -1, shortcut operand layer or None)] of every BatchNorm conv of an oracle graph."""
    unstored = _fused_away(ref.ir)
    layers = ref.ir.layers
    out = []
    for L in layers:
        if L.type != "convolutional" or not L.bn:
            continue
        i = L.index
        if i in unstored:
            S = layers[i + 1]
            assert S.type == "shortcut", (i, S.type)
            out.append((i, i + 1, i - 1, S.srcs[1]))
        else:
            out.append((i, i, i - 1, None))
    return out


def cpu_stored_layers(ref, x, upto):
    """Stored layers of a CPU walk in this mode's model up to BatchNorm conv ``upto`` of a probe (whose layers up to there are
    all BatchNorm convs): index -> float64 tensor, -1 the network input.  For the CPU demonstration that the gate catches the
    planted defects; the GPU tests feed the GPU's own stored layers instead."""
    out = {-1: x.double()}
    for c, s, src, r in bn_layers(ref):
        if c > upto:
            break
        out[s] = bn_layer_model(ref.ir.layers[c], ref.params[c], out[src], None if r is None else out[r])["model"]
    return out
