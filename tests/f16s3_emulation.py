"""CPU model of the split-f16 precision mode (precision 1, Darknet.precision = "f16s3") in float64, and the layer-local gate
built on it.

The model walks the oracle's IR with the oracle's parameters (oracle/darknet_ref.py), like tests/f16_emulation.py, and states
what the FORMAT defines, free of any summation order:

* a stored activation is a = (hi + lo) / 8 with hi = RNE_f16(clamp(8 x)), lo = RNE_f16(clamp(8 x) - hi), clamp to the f16 range
  (split_f16, csrc/rtod_internal.h).  hi + lo is exact in float32, so a value read back with read_layer IS that sum; a consumer
  re-splits it by the same rule.  A value on an exact tie of the hi rounding may re-split into another (hi, lo) pair with the
  same sum than the one the producer stored: that changes only the al*wl term the format drops, far below every floor here;
* conv weights: BatchNorm folded as plan.cpp's load_weights folds it (double arithmetic, then float: f16_emulation's
  folded_f16_weights restates it), each output channel pre-scaled by 2^e so that max |w| lies in [2^12, 2^13), then hi / lo planes
  by the same split (RNE, subnormal halves included), no clamp;
* the product sum of a conv is ah*wh + ah*wl + al*wh, evaluated here as three float64 convolutions (products of two halves are
  exact in float64, the sums carry 2^-53); al*wl is absent by definition of the format;
* layer 0 on the split stem kernel (3x3, pad 1, 32 or 64 filters; 16 filters under option stem_pool) splits 8 x in the kernel and
  runs the same three products against split weights.  Any other layer 0 runs on the exact-fp32 kernel and only STORES in the
  split format: the model then is the float64 convolution with the folded float32 weights;
* epilogue in float64: inverse pre-scale (exact), bias, linear / leaky (slope float32(0.1), the oracle's and the kernels'
  constant) / SiLU, a fused shortcut adds the operand's hi + lo, then the store split;
* routes, max-pools and nearest upsampling move stored values: the same bits.  Bilinear upsampling and a stand-alone shortcut
  add round once, at their store.

Per stored conv layer ``forward(..., records=True)`` also returns
* D = conv(|a|, |folded w|) + |bias| + |shortcut operand| in float64: the unit of every distance (r = (value - model) / D);
* with ``references=True`` float32 evaluations of the same layer from the same inputs and the same folded float32 weights, each
  followed by the same float32 epilogue and store split: torch's conv on NCHW, on channels_last, and float32 accumulation of
  32-channel K chunks in the kernels' K order (channel chunk outer, tap inner: plan.cpp load_weights; narrow Cin = 16 layers
  tap-major in chunks of two taps), per slice and then over slices where the layer is K-sliced.  Their distances to the model
  are what legitimate float32 summation orders give: the floors of the gate.

``feed`` evaluates every layer from another implementation's stored inputs (the GPU's), like F16Emulation's.
``rounding=False`` evaluates a * w in float64 with the double-folded weights and no store rounding: the oracle's arithmetic in
float64 through this walk.  ``all_terms=True, store_rounding=False`` keeps the planes and adds al*wl.
``mutant=(name, conv layer)`` plants one defect in the model (MUTANTS): tests/test_f16s3_emulation_host.py requires the gate to
catch each of them on every probe.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from f16_emulation import _fused_away
from rect_ref import predict_transform_rect, predict_transform_v5_rect

F16_MAX = 65504.0
SCALE = 8.0
LEAKY = float(np.float32(0.1))
GATE_M = 4.0          # spread between legitimate float32 summation orders of one layer (measured on the CPU: within about 4x of each other)

MUTANTS = ("ahwl_tap_or_chunk", "alwh_first32", "ahwl_last16_of_chunk", "shortcut_lo", "out_lo_group", "m_tail_chunk")


def split_planes(v8):
    """(hi, lo) float64 planes of ``v8`` (float64 or float32, already times 8): split_f16 with its saturation.  split_f16 takes a
    float32, so a float64 value is rounded to float32 once, first; v - hi is then exact in float32 and hi + lo fits one."""
    vc = v8.double().clamp(-F16_MAX, F16_MAX).float()
    hi = vc.half().float()
    lo = (vc - hi).half().float()
    return hi.double(), lo.double()


def store_split(x):
    """Stored value of an activation ``x`` (float64): (hi + lo) / 8."""
    hi, lo = split_planes(x * SCALE)
    return (hi + lo) / SCALE


def store_split_f32(x):
    """The same store on a float32 evaluation, in float32 arithmetic like the kernels' (v - hi is exact in float32)."""
    vc = (x * SCALE).clamp(-F16_MAX, F16_MAX)
    hi = vc.half().float()
    lo = (vc - hi).half().float()
    return ((hi.double() + lo.double()) / SCALE)


def folded_weights(p, L):
    """Folded conv parameters: v64 (double fold, not rounded), v32 (plan.cpp's float32 folded weight), bias (float32), and the
    real-unit float64 hi / lo planes of the pre-scaled f16 weights."""
    w = p["weight"].double()
    C = L.cout
    if L.bn:
        s = p["gamma"].double() / torch.sqrt(p["var"].double() + 1e-5)
        bias64 = p["beta"].double() - p["mean"].double() * s
    else:
        s = torch.ones(C, dtype=torch.float64)
        bias64 = p["bias"].double()
    v64 = w * s.view(C, 1, 1, 1)
    v32 = v64.float()
    wh = torch.empty_like(v64)
    wl = torch.empty_like(v64)
    for o in range(C):
        mx = float(v64[o].abs().max())
        e = 0
        if mx > 0.0:
            e = 13 - math.frexp(mx)[1]                     # mx * 2^e in [2^12, 2^13)
        e = max(-24, min(40, e))
        vs = (v32[o].double() * 2.0 ** e).float()          # exact (power of two)
        h = vs.half().float()
        l = (vs - h).half().float()
        wh[o] = h.double() * 2.0 ** -e
        wl[o] = l.double() * 2.0 ** -e
    return {"v64": v64, "v32": v32, "bias64": bias64, "bias32": bias64.float(), "wh": wh, "wl": wl}


def split_stem(L, options=()):
    """Does layer 0 run on a split stem kernel (plan.cpp: use_stem / use_stem16)?  Else the exact-fp32 conv stores the split format."""
    opts = dict(options)
    if L.size == 3 and L.pad == 1 and L.cin == 3 and L.cout in (32, 64):
        return True
    return bool(opts.get("stem_pool")) and L.size == 3 and L.pad == 1 and L.stride == 1 and L.cin == 3 and L.cout == 16


def slice_chunks(L, options=(), fused_decode=False):
    """K chunks per slice of a K-sliced layer (plan.cpp: split_slice_chunks under option k_slices_split), 0 when not sliced."""
    if not dict(options).get("k_slices_split") or L.index == 0 or L.cin % 32 or fused_decode:
        return 0
    n = L.cin * L.size * L.size // 32
    if L.hout * L.wout > 2704 or n < 8:
        return 0
    return 9 if n >= 32 else 4 if n >= 16 else 2


def k_chunks(L):
    """The kernels' K order as a list of chunks, each a list of (channel slice, ky, kx)."""
    k = L.size
    taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    if L.cin % 32:                                         # stem (one chunk), narrow layers (Cin 16: two taps per chunk)
        if L.cin == 16:
            return [[(slice(0, 16), *t) for t in taps[j:j + 2]] for j in range(0, len(taps), 2)]
        return None
    return [[(slice(c, c + 32), ky, kx)] for c in range(0, L.cin, 32) for ky, kx in taps]


def conv_chunked_f32(a, w, L, per_slice=0):
    """float32 accumulation of the K chunks in the kernels' order; each chunk's partial sum is torch's."""
    chunks = k_chunks(L)
    if chunks is None:
        return F.conv2d(a, w, None, L.stride, L.pad)
    ap = F.pad(a, (L.pad, L.pad, L.pad, L.pad))
    s = L.stride
    he, we = (L.hout - 1) * s + 1, (L.wout - 1) * s + 1

    def partial(ch):
        out = None
        for cs, ky, kx in ch:
            t = F.conv2d(ap[:, cs, ky:ky + he:s, kx:kx + we:s], w[:, cs, ky:ky + 1, kx:kx + 1])
            out = t if out is None else out + t
        return out

    total = None
    step = per_slice or len(chunks)
    for s0 in range(0, len(chunks), step):
        acc = None
        for ch in chunks[s0:s0 + step]:
            t = partial(ch)
            acc = t if acc is None else acc + t
        total = acc if total is None else total + acc
    return total


def _act(y, L, slope=LEAKY):
    if L.leaky:
        return torch.where(y > 0, y, y * (slope if y.dtype == torch.float64 else 0.1))
    if L.silu:
        return y * torch.sigmoid(y)
    return y


class F16S3Emulation:
    def __init__(self, ref, options=()):
        self.ref = ref
        self.ir = ref.ir
        self.options = tuple(options)
        self.unstored = _fused_away(self.ir)
        self._w = {}

    def weights(self, L):
        if L.index not in self._w:
            self._w[L.index] = folded_weights(self.ref.params[L.index], L)
        return self._w[L.index]

    # ------------------------------------------------------------------ one conv
    def _conv(self, L, a, res, rounding, all_terms, store, mutant, references, fused_decode):
        """``a``: float64 stored input (the network input for layer 0), ``res``: stored shortcut operand or None.
        -> (value float64, record or None)"""
        W = self.weights(L)
        i = L.index
        conv = lambda x, w: F.conv2d(x, w, None, L.stride, L.pad)
        bias = W["bias64"] if not rounding else W["bias32"].double()
        mut = mutant[0] if mutant is not None and mutant[1] == i else None
        exact_stem = i == 0 and not split_stem(L, self.options)
        if not rounding:
            acc = conv(a, W["v64"])
        elif exact_stem:
            acc = conv(a, W["v32"].double())
        else:
            hi, lo = split_planes(a * SCALE)
            ah, al = hi / SCALE, lo / SCALE
            wh, wl = W["wh"], W["wl"]
            k = L.size
            cy = cx = k // 2                               # the centre tap: inside the image for every pixel, one-row images included
            wl2, wh3 = wl, wh
            if mut == "ahwl_tap_or_chunk":                 # ah*wl dropped for one tap (k > 1) or one 32-channel chunk (1x1)
                wl2 = wl.clone()
                if k > 1:
                    wl2[:, :, cy, cx] = 0
                else:
                    wl2[:, :32] = 0
            elif mut == "ahwl_last16_of_chunk":            # ah*wl dropped for the last 16 of the 32 K elements of ONE chunk
                wl2 = wl.clone()
                if L.cin == 16:
                    c = k_chunks(L)[(cy * k + cx) // 2]   # narrow: the chunk's second tap
                    wl2[:, :, c[-1][1], c[-1][2]] = 0
                else:
                    wl2[:, 16:32, cy, cx] = 0
            elif mut == "alwh_first32":                    # al*wh dropped for the first 32 input channels
                wh3 = wh.clone()
                wh3[:, :32] = 0
            acc = conv(ah, wh) + conv(ah, wl2) + conv(al, wh3)
            if all_terms:
                acc = acc + conv(al, wl)
            if mut == "m_tail_chunk":                      # every term of one chunk dropped for the rows of the last 128-row M tile
                whc, wlc = torch.zeros_like(wh), torch.zeros_like(wl)
                cs = slice(0, min(32, L.cin))
                whc[:, cs, cy, cx] = wh[:, cs, cy, cx]
                wlc[:, cs, cy, cx] = wl[:, cs, cy, cx]
                part = conv(ah, whc) + conv(ah, wlc) + conv(al, whc)
                B, C, Ho, Wo = acc.shape
                M = B * Ho * Wo
                rows = torch.arange(M).view(B, 1, Ho, Wo) >= 128 * ((M - 1) // 128)
                acc = acc - part * rows
        y = _act(acc + bias.view(1, -1, 1, 1), L, LEAKY if rounding else 0.1)      # (the oracle in float64: the double 0.1)
        if res is not None:
            if mut == "shortcut_lo":                       # the shortcut operand's lo plane ignored
                y = y + split_planes(res * SCALE)[0] / SCALE
            else:
                y = y + res
        value = y
        if store and not fused_decode:
            value = store_split(y)
            if mut == "out_lo_group":                      # the lo plane of the output zeroed for one 8-channel group
                value = value.clone()
                value[:, 8:16] = split_planes(y[:, 8:16] * SCALE)[0] / SCALE
        rec = None
        if references is not None and rounding and not fused_decode:
            D = conv(a.abs(), W["v32"].double().abs()) + W["bias32"].double().abs().view(1, -1, 1, 1)
            if res is not None:
                D = D + res.abs()
            rec = {"conv": i, "model": value, "D": D, "refs": {}}
            if references:
                # the exact float64 conv of the same inputs with the folded float32 weights: what the format approximates
                ye = _act(conv(a, W["v32"].double()) + bias.view(1, -1, 1, 1), L)
                rec["exact"] = store_split(ye if res is None else ye + res)
                a32, v32, b32 = a.float(), W["v32"], W["bias32"].view(1, -1, 1, 1)
                r32 = None if res is None else res.float()
                per_slice = slice_chunks(L, self.options, fused_decode)

                def finish(acc32):
                    y32 = _act(acc32.contiguous() + b32, L)
                    if r32 is not None:
                        y32 = y32 + r32
                    return store_split_f32(y32)

                rec["refs"]["nchw"] = finish(F.conv2d(a32, v32, None, L.stride, L.pad))
                rec["refs"]["channels_last"] = finish(F.conv2d(a32.contiguous(memory_format=torch.channels_last),
                                                               v32.contiguous(memory_format=torch.channels_last), None, L.stride, L.pad))
                rec["refs"]["chunked"] = finish(conv_chunked_f32(a32, v32, L, per_slice))
                rec["k_slices"] = per_slice
        return value, rec

    # ------------------------------------------------------------------ the walk
    def forward(self, x, feed=None, keep_layers=False, rounding=True, all_terms=False, store_rounding=True, mutant=None,
                records=False, references=False):
        """-> detections (float64 decode of the head convs' unrounded outputs) [, layers] [, records].
        ``feed``: layer index -> tensor that REPLACES that layer's output for every consumer after it has been computed.
        ``records``: {stored layer index: {"conv", "model", "D", "refs"}} of every stored conv layer."""
        store = store_rounding and rounding
        r = store_split if store else (lambda t: t)
        x = x.double()
        outputs, computed, recs = {}, {}, {}
        detections = None
        pending = None                                      # (conv layer, pre-store epilogue inputs) of a conv fused into the next shortcut
        layers = self.ir.layers
        for L in layers:
            i = L.index
            if L.type == "convolutional":
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                if i in self.unstored and nxt.type == "shortcut":
                    pending = (L, x)                        # evaluated with the shortcut operand in its epilogue, below
                    outputs[i] = None
                    continue
                head = i in self.unstored                   # fused head decode: the float32 / float64 value goes to the decode unrounded
                x, rec = self._conv(L, x, None, rounding, all_terms, store, mutant, references if records else None, head)
                if rec is not None:
                    recs[i] = rec
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
                if pending is not None and pending[0].index == L.srcs[0]:
                    x, rec = self._conv(pending[0], pending[1], outputs[L.srcs[1]], rounding, all_terms, store, mutant,
                                        references if records else None, False)
                    if rec is not None:
                        recs[i] = rec
                    pending = None
                else:
                    x = r(outputs[L.srcs[0]] + outputs[L.srcs[1]])
            elif L.type == "route":
                x = outputs[L.srcs[0]] if len(L.srcs) == 1 else torch.cat([outputs[s] for s in L.srcs], 1)
            elif L.type == "yolo":
                x = (predict_transform_v5_rect if L.decode_v5 else predict_transform_rect)(x, self.ref.height, L.anchors, L.classes)
                detections = x if detections is None else torch.cat((detections, x), 1)
                outputs[i] = outputs[i - 1]
                continue
            outputs[i] = x
            if feed is not None and i in feed:
                computed[i] = x
                x = outputs[i] = feed[i].double()
        out = [detections]
        if keep_layers:
            out.append(outputs if feed is None else {**outputs, **computed})
        if records:
            out.append(recs)
        return out[0] if len(out) == 1 else tuple(out)

    __call__ = forward


# ------------------------------------------------------------------------------------- distances and the gate
def residual(value, rec):
    """r = (value - model) / D, element-wise (numpy float64)."""
    v = value.double() if isinstance(value, torch.Tensor) else torch.from_numpy(np.asarray(value, dtype=np.float64))
    return ((v - rec["model"]) / rec["D"]).numpy()


def rms_max(r):
    r = np.asarray(r, dtype=np.float64)
    return float(np.sqrt(np.mean(r * r))), float(np.abs(r).max())


def floors(rec):
    """(F_rms, F_max): the largest rms and the largest max of r over the float32 reference evaluations of the layer."""
    assert rec["refs"], "record without reference evaluations (references=True)"
    d = [rms_max(residual(v, rec)) for v in rec["refs"].values()]
    return max(a for a, _ in d), max(b for _, b in d)


def gate(r, floors_, m=GATE_M):
    """The layer-local gate: rms(r) <= m * F_rms and max|r| <= m * F_max.  -> (passed, rms / F_rms, max / F_max)"""
    f_rms, f_max = floors_
    rms, mx = rms_max(r)
    assert f_rms > 0 and f_max > 0, (f_rms, f_max)
    return (rms <= m * f_rms and mx <= m * f_max), rms / f_rms, mx / f_max
