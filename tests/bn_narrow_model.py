"""Narrow square probes and the layer-local float64 model of batch-statistics BatchNorm on the narrow split-f16 kernels (plan
options bn_batch_stats + bn_batch_split + bn_split_narrow, precision 1).  Test helper of tests/test_bn_narrow_host.py and
tests/test_bn_narrow_gpu.py; extends tests/bn_split_model.py.

Probes (conv_probes.Probe with a 16-filter stem; the conv under test is layer 1 and reads the stem's 16 channels):

* n_c32:   16 -> 32, 3x3 stride 1, 12x12, B = 3: 144 pixels per frame, so every M tile holds a frame boundary and a ragged tail;
* n_c24s2: 16 -> 24, 3x3 stride 2, 22x22 -> 11x11, B = 3: 256 % (24 / 4) != 0, the one-stage statistics.  No conv may read 24
  channels, so an 8-filter sibling (also Cin 16, stride 2) fills the concat to 32 for the head;
* n_c16pw: 16 -> 16, 1x1, 14x14, B = 3 (the head then reads 16 channels: a narrow conv without BatchNorm, fused decode).

``narrow_layer_model`` is bn_split_model.bn_layer_model plus
* layer 0 on the 16-filter split stem (option stem_pool, ``split_stem=True``): the three products xh*wh + xh*wl + xl*wh of the split
  of 8 x against the split UNFOLDED weights, like every later BatchNorm conv (without stem_pool: the exact-fp32 conv, as before);
* ``pooled=True``: the record of the pooled pair — the 2x2 / stride-2 max-pool of the modelled stored values ("pool_model"), the unit
  D at the model's winners ("pool_D"), the pooled float32 references ("pool_refs"): what normalise + pool in one kernel must store.

MUTANTS (each planted in the model; the host test requires the gate to catch it):
* stats_after_pool: the statistics taken over the pooled raw map (a fused kernel that reduced what it stored);
* pool_hi_only:     the window's winner chosen on the hi halves alone (the first of equal hi wins, whatever its lo);
* stem_lo_dropped:  xl*wh missing on layer 0.

``mean_tolerance``: bound on |batch mean - model mean| per channel from the format alone.  A raw sum is a chain of fp32 additions
of exact f16 x f16 products: one MFMA accumulation per product and 32-wide K chunk (three per chunk in the split arithmetic, K + 1
steps on the exact-fp32 kernel), each rounding once relative to a partial sum bounded by conv(|a|, |w|); the undo of the power-of-two
pre-scale is exact and the statistics are double sums of those float32 values.  So
|mean error| <= (steps + 2) 2^-24 mean(conv(|a|, |w|)): no summation order can exceed it, a statistic over the wrong set of pixels does.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from bn_split_model import EPS, _act, _stats, bn_layers
from conv_probes import CLASSES, Probe
from f16s3_emulation import SCALE, conv_chunked_f32, folded_weights, split_planes, store_split, store_split_f32
from realtimeobjectdetection_amd.cfgs import _ANCHORS_V3, _conv, _net, _route, _yolo

NARROW_OPTIONS = (("narrow_cin", 1), ("stem_pool", 1), ("bn_batch_stats", 1), ("bn_batch_split", 1), ("bn_split_narrow", 1))
MUTANTS = ("stats_after_pool", "pool_hi_only", "stem_lo_dropped")


class SiblingProbe(Probe):
    """A probe whose conv under test has a channel count no conv can read (24): an 8-filter sibling fills the concat to 32."""

    @property
    def has_1x1(self):
        return False

    def cfg(self):
        L = _net(self.H, self.W)
        L += _conv(self.stem, 3, 1)                                  # 0
        L += _conv(self.cout, self.k, self.stride, act=self.act)     # 1: the conv under test
        L += _route(-2)                                              # 2: the stem again
        L += _conv(32 - self.cout, self.k, self.stride)              # 3: the sibling
        L += _route(-1, 1)                                           # 4: sibling + conv under test, 32 channels, zero-copy
        L += _conv(3 * (5 + CLASSES), 1, 1, bn=False, act="linear") + _yolo((0, 1, 2), _ANCHORS_V3, 9, CLASSES)
        return "\n".join(L) + "\n"


def _p(cls, name, shape, B, note):
    return cls(name, *shape, B, note=note, options=NARROW_OPTIONS)


NARROW = [
    _p(Probe, "n_c32", (12, 12, 16, 32, 3, 1), 3, "144 pixels per frame: a frame boundary and a ragged tail in every M tile"),
    _p(SiblingProbe, "n_c24s2", (22, 22, 16, 24, 3, 2), 3, "stride 2 onto 11x11; Cout 24: one-stage statistics, coff 8 of a concat"),
    _p(Probe, "n_c16pw", (14, 14, 16, 16, 1, 1), 3, "1x1: one K chunk, its second tap absent"),
]
BY_NAME = {p.name: p for p in NARROW}


def _pool_pick(v, key):
    """2x2 / stride-2 windows of ``v`` scanned in (dy, dx) order: the element whose ``key`` is the first strict maximum."""
    B, C, H, W = v.shape
    win = lambda t: torch.stack([t[:, :, dy:H:2, dx:W:2] for dy in (0, 1) for dx in (0, 1)], 0)
    idx = win(key).argmax(0, keepdim=True)        # torch.argmax returns the first maximal index: "replace only when strictly greater"
    return win(v).gather(0, idx)[0], idx


def narrow_layer_model(L, p, a, res, mutant=None, references=False, split_stem=False, pooled=False):
    """Record of BatchNorm conv ``L`` from stored input ``a`` (the network input for layer 0) and shortcut operand ``res``:
    {"conv", "model", "D", "refs", "mean", "var", "Dconv_mean", "steps"} and, with ``pooled``, {"pool_model", "pool_D", "pool_refs"}."""
    assert L.bn
    a = a.double()
    res = None if res is None else res.double()
    w32 = p["weight"].float()
    conv = lambda x, w: F.conv2d(x, w, None, L.stride, L.pad)
    K = L.cin * L.size * L.size
    if L.index == 0 and not split_stem:                        # exact-fp32 kernel
        raw = conv(a, w32.double())
        steps = K + 1
    else:
        W = folded_weights({"weight": p["weight"], "bias": torch.zeros(L.cout)}, SimpleNamespace(bn=False, cout=L.cout))
        hi, lo = split_planes(a * SCALE)
        ah, al = hi / SCALE, lo / SCALE
        raw = conv(ah, W["wh"]) + conv(ah, W["wl"])
        if not (mutant == "stem_lo_dropped" and L.index == 0):
            raw = raw + conv(al, W["wh"])
        steps = 3 * math.ceil((32 if L.index == 0 else K) / 32)
    gamma, beta = p["gamma"].double().view(1, -1, 1, 1), p["beta"].double().view(1, -1, 1, 1)
    if mutant == "stats_after_pool":
        mean, var = _stats(F.max_pool2d(raw, 2, 2))
    else:
        mean, var = _stats(raw)
    wc = gamma / torch.sqrt(var + EPS)
    bc = beta - mean * wc
    y = _act(raw * wc + bc, L)
    if res is not None:
        y = y + res
    Dconv = conv(a.abs(), w32.double().abs())
    D = wc.abs() * Dconv + beta.abs()
    if res is not None:
        D = D + res.abs()
    rec = {"conv": L.index, "model": store_split(y), "D": D, "refs": {}, "mean": mean.flatten(), "var": var.flatten(),
           "Dconv_mean": Dconv.mean((0, 2, 3)), "steps": steps}
    if references:
        a32 = a.float()
        r32 = None if res is None else res.float()

        def finish(raw32):
            raw32 = raw32.contiguous()
            m, v = _stats(raw32)                               # double statistics of the float32 sums
            invstd = 1.0 / torch.sqrt(v + EPS)
            w = (invstd * gamma).float()                       # the kernels' per-channel constants (bn_apply_kernel)
            b = (beta - m * invstd * gamma).float()
            y32 = _act(raw32 * w + b, L)
            if r32 is not None:
                y32 = y32 + r32
            return store_split_f32(y32)

        rec["refs"]["nchw"] = finish(F.conv2d(a32, w32, None, L.stride, L.pad))
        rec["refs"]["channels_last"] = finish(F.conv2d(a32.contiguous(memory_format=torch.channels_last),
                                                       w32.contiguous(memory_format=torch.channels_last), None, L.stride, L.pad))
        rec["refs"]["chunked"] = finish(conv_chunked_f32(a32, w32, L))
    if pooled:
        m = rec["model"]
        key = split_planes(m * SCALE)[0] if mutant == "pool_hi_only" else m
        rec["pool_model"], idx = _pool_pick(m, key)
        B, C, H, W = D.shape
        rec["pool_D"] = torch.stack([D[:, :, dy:H:2, dx:W:2] for dy in (0, 1) for dx in (0, 1)], 0).gather(0, idx)[0]
        rec["pool_refs"] = {k: F.max_pool2d(v, 2, 2) for k, v in rec["refs"].items()}
    return rec


def pool_record(rec):
    """The pooled pair of a ``pooled`` record in the shape f16s3_emulation.residual / floors / gate take."""
    return {"model": rec["pool_model"], "D": rec["pool_D"], "refs": rec["pool_refs"]}


def mean_tolerance(rec):
    """Per-channel bound on |batch mean - rec["mean"]| (module docstring)."""
    return (rec["steps"] + 2) * 2.0 ** -24 * rec["Dconv_mean"]


def stem_is_split(ir, options):
    """Does layer 0 run the 16-filter split stem (plan.cpp use_stem16 under option stem_pool)?"""
    L = ir.layers[0]
    return bool(dict(options).get("stem_pool")) and L.size == 3 and L.stride == 1 and L.pad == 1 and L.cin == 3 and L.cout == 16


def cpu_stored(ref, x, upto, options=NARROW_OPTIONS):
    """Stored layers of a CPU walk of this mode's model over the leading BatchNorm convs and 2x2 / stride-2 max-pools of a graph,
    up to layer ``upto``: index -> float64 tensor, -1 the network input."""
    out = {-1: x.double()}
    split0 = stem_is_split(ref.ir, options)
    for L in ref.ir.layers[:upto + 1]:
        i = L.index
        if L.type == "convolutional":
            assert L.bn
            out[i] = narrow_layer_model(L, ref.params[i], out[i - 1], None, split_stem=split0)["model"]
        else:
            assert L.type == "maxpool" and L.size == 2 and L.stride == 2
            out[i] = F.max_pool2d(out[i - 1], 2, 2)
    return out

