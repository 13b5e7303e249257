"""CPU emulation of the plain-f16 precision mode (precision 2, Darknet.precision = "f16") on torch float32 ops.

It walks the oracle's IR with the oracle's parameters (oracle/darknet_ref.py) and rounds where the GPU plan rounds:
* conv weights: BatchNorm folded as plan.cpp's layout_weights folds it (double arithmetic, then float), each output channel
  pre-scaled by 2^e so that its max |w| lies in [2^12, 2^13), rounded to f16 (RNE), scaled back (exact);
* every STORED activation: RNE_f16(8 x) / 8, saturated at the f16 range like the kernels' stores.  A conv whose output feeds only
  a fused shortcut or a fused head decode is not stored: the shortcut sum is rounded once, the decode reads the fp32 value;
* layer 0 (the split stem) convolves the fp32 input with the exact folded weights, then rounds its output like any store.
Convolutions accumulate in float32 (torch CPU), which is what the f16 MFMA's fp32 accumulator does up to summation order.

``feed`` evaluates every layer from another implementation's stored inputs (the GPU's, tests/test_f16_gpu.py): the distance
then measures that layer's arithmetic alone, not the rounding history of everything before it.
``rounding=False`` evaluates the oracle's own ops (conv -> batch_norm -> activation) through the same layer walk, which must give
the oracle's bits (tests/test_f16_host.py): the walk, the fusion bookkeeping and the decode are then the oracle's.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import darknet_ref as O

F16_MAX = 65504.0
SCALE = 8.0


def round_act(x: torch.Tensor) -> torch.Tensor:
    """Stored value of an activation in an f16 plan: RNE_f16(8 x) / 8 with the kernels' saturation."""
    return (x * SCALE).clamp(-F16_MAX, F16_MAX).half().float() / SCALE


def folded_f16_weights(p, L, rounding=True):
    """(weight, bias) of one conv with BatchNorm folded like plan.cpp (load_weights), weights rounded to the f16 hi plane."""
    w = p["weight"].double()
    C = L.cout
    if L.bn:
        s = p["gamma"].double() / torch.sqrt(p["var"].double() + 1e-5)
        bias = (p["beta"].double() - p["mean"].double() * s).float()
    else:
        s = torch.ones(C, dtype=torch.float64)
        bias = p["bias"].float()
    v = (w * s.view(C, 1, 1, 1)).float()                   # the fp32 folded weight
    if not rounding:
        return v, bias
    out = torch.empty_like(v)
    for o in range(C):
        mx = float(v[o].abs().max())
        e = 0
        if mx > 0.0:
            e = 13 - math.frexp(mx)[1]                     # mx * 2^e in [2^12, 2^13)
        e = max(-24, min(40, e))
        hi = (v[o].double() * 2.0 ** e).float().half()     # RNE, subnormals included
        out[o] = (hi.double() * 2.0 ** -e).float()         # exact
    return out, bias


def _fused_away(ir):
    """Conv layers whose output the plan never stores: sole producer of a following shortcut (srcs[0]) or of a yolo head."""
    cons = {}
    for L in ir.layers:
        if L.type in ("convolutional", "upsample", "maxpool", "yolo") and L.index > 0:
            cons.setdefault(L.index - 1, []).append(L.index)
        elif L.type in ("shortcut", "route"):
            for s in L.srcs:
                cons.setdefault(s, []).append(L.index)
    out = set()
    for L in ir.layers:
        i = L.index
        if L.type != "convolutional" or len(cons.get(i, [])) != 1:
            continue
        nxt = ir.layers[i + 1] if i + 1 < len(ir.layers) else None
        if nxt is None or cons[i][0] != i + 1:
            continue
        if nxt.type == "shortcut" and nxt.srcs[1] != i:
            out.add(i)
        elif nxt.type == "yolo" and not cons.get(i + 1):
            out.add(i)
    return out


class F16Emulation:
    def __init__(self, ref: O.RefDarknet):
        self.ref = ref
        self.ir = ref.ir
        self.unstored = _fused_away(self.ir)
        self._w = {}

    def _weights(self, L, rounding):
        key = (L.index, rounding)
        if key not in self._w:
            self._w[key] = folded_f16_weights(self.ref.params[L.index], L, rounding and L.index > 0)
        return self._w[key]

    def forward(self, x: torch.Tensor, rounding=True, keep_layers=False, feed=None):
        """``feed``: layer index -> tensor that REPLACES that layer's output for every consumer after it has been computed
        (layer-local evaluation: each layer from another implementation's materialised inputs)."""
        r = round_act if rounding else (lambda t: t)
        computed = {}
        outputs = {}
        detections = None
        for L in self.ir.layers:
            i = L.index
            if L.type == "convolutional":
                if rounding:
                    w, b = self._weights(L, True)
                    x = F.conv2d(x, w, b, L.stride, L.pad)
                else:
                    p = self.ref.params[i]
                    x = F.conv2d(x, p["weight"], p.get("bias"), L.stride, L.pad)
                    if L.bn:
                        x = F.batch_norm(x, p["mean"], p["var"], p["gamma"], p["beta"], training=False, momentum=0.1, eps=1e-5)
                if L.leaky:
                    x = F.leaky_relu(x, 0.1)
                elif L.silu:
                    x = F.silu(x)
                if i not in self.unstored:
                    x = r(x)
            elif L.type == "upsample":
                if L.nearest:
                    x = F.interpolate(x, scale_factor=2, mode="nearest")
                else:
                    x = r(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))
            elif L.type == "maxpool":
                if L.pool_pad:
                    x = F.max_pool2d(x, L.size, L.stride, L.pool_pad)
                elif L.stride != 1:
                    x = F.max_pool2d(x, L.size, L.stride)
                else:
                    x = F.pad(x, (0, L.size - 1, 0, L.size - 1), mode="replicate")
                    x = F.max_pool2d(x, L.size, L.size - 1)
            elif L.type == "shortcut":
                x = r(outputs[L.srcs[0]] + outputs[L.srcs[1]])
            elif L.type == "route":
                x = outputs[L.srcs[0]] if len(L.srcs) == 1 else torch.cat([outputs[s] for s in L.srcs], 1)
            elif L.type == "yolo":
                x = (O.predict_transform_v5 if L.decode_v5 else O.predict_transform)(x, self.ref.height, L.anchors, L.classes)
                detections = x if detections is None else torch.cat((detections, x), 1)
                outputs[i] = outputs[i - 1]
                continue
            outputs[i] = x
            if feed is not None and i in feed:
                computed[i] = x
                x = outputs[i] = feed[i]
        if keep_layers:
            return detections, (outputs if feed is None else {**outputs, **computed})
        return detections

    __call__ = forward


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def layer_distance(got, ref):
    """Per-layer distances: max |got - ref| / max(1, max |ref|), and rms(got - ref) / max(1e-30, rms(ref))."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    d = got - ref
    return {"max_over_absmax": float(np.abs(d).max() / max(1.0, np.abs(ref).max())),
            "rms_rel": float(np.sqrt(np.mean(d * d)) / max(1e-30, np.sqrt(np.mean(ref * ref))))}


def output_distance(got, ref):
    e = rel(got, ref)
    return {"p999": float(np.quantile(e, 0.999)), "max": float(e.max()),
            "rms_rel": float(np.sqrt(np.mean((np.asarray(got, np.float64) - np.asarray(ref, np.float64)) ** 2)) /
                             np.sqrt(np.mean(np.asarray(ref, np.float64) ** 2)))}
