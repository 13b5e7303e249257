"""Host-side mirror of the reference's ``Darknet`` class, backed by librtod.so.

Drop-in surface (reference: src/darknet.py:138-603, SURVEY.md §8 b): ``Darknet(cfg_file_path, CUDA)``,
``.blocks`` / ``.net_info`` (mutable; callers set ``net_info["height"]``) / ``.module_list`` /
``.header`` / ``.seen`` / ``.CUDA`` / ``.TRAIN``, (extension) ``.input_width`` for rectangular inputs, ``get_blocks()``, ``get_module_list()``,
``load_weights(path)``, ``load_state_dict`` with the reference's key names
(``module_list.{i}.conv_{i}.weight`` ...), ``forward(x) -> [B,N,5+C]``, ``train_mode()``, and after
the first forward ``.anchors`` / ``.num_classes``.

Everything numeric happens in hand-written HIP kernels behind the C ABI (include/rtod.h).  The
``nn.Module`` tree only *holds* the parameters in the reference's layout so ``state_dict`` /
``.parameters()`` / ``.cuda()`` keep working; PyTorch executes none of the network.  There is no
CPU fallback: a non-CUDA input or a missing librtod.so raises.

BatchNorm follows the module's mode like ``nn.BatchNorm2d``: ``.eval()`` = running statistics folded into the
convolutions — the canonical, fast, frame-independent mode of SURVEY.md F2.  The reference's callers never call
``.eval()``, so there BN uses batch statistics (frames of a batch influence each other); a model left in training
mode runs exactly that on the exact-fp32 kernels (a slow parity path, with a one-time warning) unless
``bn_running_stats_in_train`` asks for eval semantics regardless of the mode.
"""
import ctypes as C
import json
import os
import warnings
import weakref
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import torch
import torch.nn as nn

from . import _ffi
from .cfg import parse_cfg, build_ir


_OVERFLOW_MSG = ("Darknet (precision f16s3 / f16): an activation reached the split-f16 range limit (|x| >= 8188) and was saturated; "
                 "the results of that forward are not valid. Use precision='fp32' (exact MFMA kernels) for these weights.")


# The three kinds of trained conv, stated once: what ``Darknet._step`` / ``_update`` / ``sync_stepped_parameters`` and train.py read.
#   bn      the layer has BatchNorm (what ``_trained_conv`` holds it to)
#   params  its trained parameters, by the names the trainer uses; ``attrs``: the (module, attribute) each lives in
#   step, update   the two doors of the kind; their C entries are "rtod_plan_" + the door's name.  The update entry takes the new
#           values in the order of ``params``
#   order   the order in which the step door and its C entry take masters ("name") and gradients ("d.name"); the moments follow,
#           (exp_avg, exp_avg_sq) per parameter in the order of ``params``, NULL for SGD
#   moments, takes, update_got   the kind's own words in the error texts
ConvKind = namedtuple("ConvKind", "bn params attrs step update order moments takes update_got")
CONV_KINDS = {
    "head": ConvKind(False, ("weight", "bias"), (("conv", "weight"), ("conv", "bias")), "step_conv", "update_conv",
                     ("weight", "bias", "d.weight", "d.bias"), "(exp_avg_w, exp_avg_sq_w, exp_avg_b, exp_avg_sq_b)",
                     "weight %(weight)s and bias %(channels)s", True),
    "folded": ConvKind(True, ("weight",), (("conv", "weight"),), "step_conv_folded", "update_conv_weight",
                       ("weight", "d.weight"), "(exp_avg, exp_avg_sq)", "weight %(weight)s", True),
    "bn": ConvKind(True, ("weight", "gamma", "beta"), (("conv", "weight"), ("bn", "weight"), ("bn", "bias")), "step_conv_bn", "update_conv_bn",
                   ("weight", "d.weight", "gamma", "beta", "d.gamma", "d.beta"),
                   "(exp_avg_w, exp_avg_sq_w, exp_avg_gamma, exp_avg_sq_gamma, exp_avg_beta, exp_avg_sq_beta)",
                   "weight %(weight)s, gamma and beta [%(cout)d]", False),
}


def take_pending_overflow(prediction):
    """``(model, flag tensor)`` of the forward that produced ``prediction`` (or ``(None, None)``): util.write_results reads the
    flag in the same host synchronisation as its detection counts instead of paying a second round trip.  The link is a tag on
    the output tensor OBJECT itself — (weak reference to the model, its forward sequence number), set by Darknet.forward —
    not the tensor's address: a freed-and-reused address can no longer attach a stale model to another tensor."""
    tag = getattr(prediction, "_rtod_forward", None)
    if tag is None:
        return None, None
    prediction._rtod_forward = None                            # consumed: a second write_results on the same tensor reads nothing
    model = tag[0]()
    if model is None or model._ovf is None:
        return None, None
    return model, model._ovf


def raise_overflow(model):
    model._ovf.zero_()
    raise FloatingPointError(_OVERFLOW_MSG)


class EmptyLayer(nn.Module):
    """Placeholder for route / shortcut blocks (reference: src/darknet.py:49-54)."""


class DetectionLayer(nn.Module):
    """Holds the masked anchors of a yolo block (reference: src/darknet.py:57-97)."""

    def __init__(self, anchors, CUDA=False):
        super().__init__()
        self.anchors = anchors
        self.CUDA = CUDA


class MaxPoolStride1(nn.Module):
    """Marker for ``[maxpool] stride=1`` (reference: src/darknet.py:17-46); executed by librtod."""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        self.pad = kernel_size - 1


def _blocks_to_cfg_text(blocks) -> str:
    """Serialise parsed blocks back to cfg text for the native parser (route ``layers`` may have
    been split into a list by create_modules, as in the reference, src/darknet.py:564)."""
    out = []
    for b in blocks:
        out.append("[%s]" % b["type"])
        for k, v in b.items():
            if k == "type":
                continue
            if isinstance(v, (list, tuple)):
                v = ",".join(str(a) for a in v)
            out.append("%s=%s" % (k, v))
        out.append("")
    return "\n".join(out) + "\n"


class Darknet(nn.Module):
    def __init__(self, cfg_file_path, CUDA):
        super().__init__()
        self.blocks = self.parse_cfg(cfg_file_path)
        self.net_info, self.module_list = self.create_modules(self.blocks)
        self.header = torch.IntTensor([0, 0, 0, 0])
        self.seen = 0
        self.CUDA = CUDA
        self.TRAIN = False
        self.bn_running_stats_in_train = False
        self._warned_batch_bn = False
        self.update_running_stats = True   # training-mode forward updates running_mean / running_var / num_batches_tracked like torch does
        # "fp32" (exact MFMA) | "f16s3" (split f16, 3 products) | "auto" (f16s3 where the cfg allows it, else fp32) |
        # "f16" (opt-in plain f16, one product: faster, ~1e-3 relative error; never chosen by "auto")
        self.precision = os.environ.get("RTOD_PRECISION", "auto")
        self.keep_all_layers = False      # debug: no activation-arena reuse (read_layer after forward)
        # None: square input net_info["height"] x net_info["height"] (the reference's calling sequence).  An int: opt-in rectangular
        # input [B,3,net_info["height"],input_width] (rtod_plan_create_rect; every head needs one integer stride on both axes)
        self.input_width = None
        self.autotune = True              # split-f16 plans: measure the tile variants once per batch size (rtod_plan_autotune)
        self.options = {}                 # rtod_plan_set_option name -> int (fusion / kernel-selection switches, tests and A/B runs)
        # split-f16 range guard (|activation| < 8188): producers saturate and raise a device flag.  "write_results": the flag
        # is read at write_results' existing host sync; "forward": read (one host sync) after every forward, and with
        # precision "auto" the plan falls back to the exact-fp32 kernels and re-runs; "off": never read.
        self.overflow_check = "write_results"
        self._ovf = None
        self._forward_seq = 0             # forwards whose range flag is still to be read (tag on the output tensor, see take_pending_overflow)
        self._tuned = set()
        self._cfg_text = _blocks_to_cfg_text(self.blocks)
        self._plan = None
        self._plan_key = None
        self._weights_version = 0
        self._stats_version = 0             # running_mean / running_var updates of training-mode forwards (eval plans fold them)
        self._plan_weights_version = -1
        self._info = None
        self._stepped = {}                  # _step: {conv layer: (kind, its masters in the order of the kind's params)} the module's parameters lag behind

    # ------------------------------------------------------------------ reference getters
    def get_blocks(self) -> list:
        return self.blocks

    def get_module_list(self) -> nn.ModuleList:
        return self.module_list

    @staticmethod
    def parse_cfg(cfg_file_path):
        return parse_cfg(cfg_file_path)

    @staticmethod
    def create_modules(blocks):
        """Same module tree / parameter names as the reference builds (src/darknet.py:449-603) so
        state_dicts are interchangeable; shapes come from the shared IR."""
        net_info = blocks[0]
        ir = build_ir(blocks, int(net_info.get("height", 416)))
        module_list = nn.ModuleList()
        for L, blk in zip(ir.layers, blocks[1:]):
            i = L.index
            m = nn.Sequential()
            if L.type == "convolutional":
                m.add_module("conv_%d" % i, nn.Conv2d(L.cin, L.cout, L.size, L.stride, L.pad, bias=not L.bn))
                if L.bn:
                    m.add_module("batch_norm_%d" % i, nn.BatchNorm2d(L.cout))
                if L.leaky:
                    m.add_module("leaky_%d" % i, nn.LeakyReLU(0.1, inplace=True))
                elif L.silu:                                   # cfg extension (activation=silu)
                    m.add_module("silu_%d" % i, nn.SiLU(inplace=True))
            elif L.type == "upsample":
                if L.nearest:                                  # cfg extension (mode=nearest)
                    m.add_module("upsample_%d" % i, nn.Upsample(scale_factor=2, mode="nearest"))
                else:
                    m.add_module("upsample_%d" % i, nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
            elif L.type == "route":
                if isinstance(blk["layers"], str):
                    blk["layers"] = blk["layers"].split(",")        # the reference splits in place
                m.add_module("route_%d" % i, EmptyLayer())
            elif L.type == "shortcut":
                m.add_module("shortcut_%d" % i, EmptyLayer())
            elif L.type == "maxpool":
                if L.pool_pad:                                 # cfg extension (symmetric=1)
                    m.add_module("maxpool_%d" % i, nn.MaxPool2d(L.size, L.stride, L.pool_pad))
                else:
                    m.add_module("maxpool_%d" % i, nn.MaxPool2d(L.size, L.stride) if L.stride != 1 else MaxPoolStride1(L.size))
            elif L.type == "yolo":
                m.add_module("Detection_%d" % i, DetectionLayer([tuple(a) for a in L.anchors]))
            module_list.append(m)
        return net_info, module_list

    # ------------------------------------------------------------------ weights
    def configure_weights(self, weight_file_path):
        with open(weight_file_path, "rb") as fp:
            header = np.fromfile(fp, dtype=np.int32, count=5)
            weights = np.fromfile(fp, dtype=np.float32)
        self.header = torch.from_numpy(header)
        self.seen = self.header[3]
        return weights

    def load_weights(self, weight_file_path: str):
        """Darknet binary -> module tensors (reference: src/darknet.py:316-410)."""
        w = self.configure_weights(weight_file_path)
        self.load_weight_stream(w)

    def load_weight_stream(self, w: np.ndarray):
        ptr = 0
        self._stepped.clear()                                     # every parameter is replaced: nothing lags any more
        with torch.no_grad():
            for m in self.module_list:
                conv = bn = None
                for name, sub in m.named_children():
                    if name.startswith("conv_"):
                        conv = sub
                    elif name.startswith("batch_norm_"):
                        bn = sub
                if conv is None:
                    continue
                c = conv.out_channels
                if bn is not None:
                    for t in (bn.bias, bn.weight, bn.running_mean, bn.running_var):
                        t.copy_(torch.from_numpy(w[ptr:ptr + c]).view_as(t)); ptr += c
                else:
                    conv.bias.copy_(torch.from_numpy(w[ptr:ptr + c]).view_as(conv.bias)); ptr += c
                n = conv.weight.numel()
                conv.weight.copy_(torch.from_numpy(w[ptr:ptr + n]).view_as(conv.weight)); ptr += n
        self._weights_version += 1
        return ptr

    def weight_stream(self) -> np.ndarray:
        """Current parameters as a ``.weights`` float payload (host, float32).  Convs stepped on the device (``step_conv``) are
        brought up to date first (``sync_stepped_parameters``), so the stream — and every re-pack, which reads it — holds them."""
        self.sync_stepped_parameters()
        parts = []
        for layer in range(len(self.module_list)):
            conv, bn = self._conv_bn(layer)
            if conv is None:
                continue
            if bn is not None:
                parts += [bn.bias, bn.weight, bn.running_mean, bn.running_var]
            else:
                parts.append(conv.bias)
            parts.append(conv.weight)
        return np.concatenate([p.detach().float().cpu().numpy().reshape(-1) for p in parts]).astype(np.float32, copy=False)

    def load_state_dict(self, *args, **kwargs):
        self.sync_stepped_parameters()                            # a partial (strict=False) dict keeps the stepped convs it does not name
        r = super().load_state_dict(*args, **kwargs)
        self._weights_version += 1
        return r

    def state_dict(self, *args, **kwargs):
        self.sync_stepped_parameters()
        return super().state_dict(*args, **kwargs)

    def invalidate_weights(self):
        """Call after mutating parameters in place so the next forward re-packs them.  Convs stepped on the device are brought up
        to date first (mutate after this call's predecessors, not between ``step_conv`` and it: the masters would win)."""
        self.sync_stepped_parameters()
        self._weights_version += 1

    # ------------------------------------------------------------------ detection heads
    def head_layers(self) -> list:
        """``[(conv_layer, input_layer)]`` of the detection heads in cfg order: the conv directly in front of every [yolo] block
        and the layer whose output it reads (what ``read_layer`` returns after a forward with options ``keep_head_inputs``)."""
        types = [b["type"] for b in self.blocks[1:]]
        return [(i - 1, i - 2) for i, t in enumerate(types) if t == "yolo" and i > 0 and types[i - 1] == "convolutional"]

    def update_conv(self, layer: int, weight, bias) -> None:
        """Replace the weights of one conv without BatchNorm: ``weight`` [Cout,Cin,k,k] and ``bias`` [Cout] go into the module's
        parameters and, when a plan with current weights is loaded, into that plan through rtod_plan_update_conv, which re-packs
        this conv alone (the bits a full re-pack gives) — the next forward does not re-pack the network.  Synchronises."""
        self._update("head", layer, (weight, bias))

    # ---- what the six doors of the three kinds of trained conv (CONV_KINDS) share
    def _conv_bn(self, layer):
        """``(conv, batch_norm)`` modules of a layer, None for what it does not have (or for a layer out of range)."""
        conv = bn = None
        if 0 <= int(layer) < len(self.module_list):
            for name, sub in self.module_list[int(layer)].named_children():
                if name.startswith("conv_"):
                    conv = sub
                elif name.startswith("batch_norm_"):
                    bn = sub
        return conv, bn

    def _trained_conv(self, who, layer, with_bn):
        conv, bn = self._conv_bn(layer)
        if conv is None or (bn is not None) != with_bn:
            raise ValueError("Darknet.%s: layer %d is not a convolution %s BatchNorm" % (who, int(layer), "with" if with_bn else "without"))
        return conv

    @staticmethod
    def _opt_step(opt):
        if isinstance(opt, _ffi.OptStep):
            return opt
        return _ffi.OptStep(int(opt["kind"]), float(opt["lr"]), float(opt.get("beta1", 0.0)), float(opt.get("beta2", 0.0)), float(opt.get("eps", 0.0)), int(opt.get("step", 0)))

    @staticmethod
    def _need_f32_on(who, dev, tensors):
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("Darknet.%s: every tensor must be a contiguous float32 tensor on %s" % (who, dev))

    def _params(self, kind, layer):
        """The module parameters of a conv of ``kind``, in the order of the kind's ``params``."""
        mods = dict(zip(("conv", "bn"), self._conv_bn(layer)))
        return [getattr(mods[m], a) for m, a in CONV_KINDS[kind].attrs]

    @staticmethod
    def _takes(K, conv):
        return K.takes % {"weight": tuple(conv.weight.shape), "channels": (conv.out_channels,), "cout": conv.out_channels}

    def _update(self, kind, layer, values):
        """The parameters of one conv replaced in the module and, when a plan with current weights is loaded, re-packed there alone."""
        K = CONV_KINDS[kind]
        layer = int(layer)
        conv = self._trained_conv(K.update, layer, K.bn)
        new = [(p, torch.as_tensor(t).detach().to(torch.float32)) for p, t in zip(self._params(kind, layer), values)]
        if any(tuple(t.shape) != tuple(p.shape) for p, t in new):
            got = ", got %s" % " and ".join(str(tuple(t.shape)) for _, t in new) if K.update_got else ""
            raise ValueError("Darknet.%s: layer %d takes %s%s" % (K.update, layer, self._takes(K, conv), got))
        with torch.no_grad():
            for p, t in new:
                p.copy_(t)
        self._stepped.pop(layer, None)                            # the parameters are current again
        if self._plan_is_current():
            host = [np.ascontiguousarray(t.cpu().numpy()) for _, t in new]
            with torch.cuda.device(self._plan_key[2]):
                _ffi.check(getattr(_ffi.lib(), "rtod_plan_" + K.update)(self._plan, layer, *host))
        # the plan's weight version stays current: parameters and plan agree again (a plan that was stale before still re-packs)

    def _step(self, kind, layer, opt, operands, moments):
        """One optimiser step of one conv on the current stream: masters and moments in place, the conv's block of the image
        re-packed.  ``operands``: masters and gradients in the kind's ``order``."""
        K = CONV_KINDS[kind]
        who, layer = K.step, int(layer)
        if not self._plan_is_current():
            raise RuntimeError("Darknet.%s: no loaded plan holds the current parameters; run a forward first" % who)
        dev = torch.device("cuda", self._plan_key[2])
        n_mom = 2 * len(K.params)
        if moments is not None and len(moments) != n_mom:
            raise ValueError("Darknet.%s: moments = %s" % (who, K.moments))
        mom = list(moments) if moments is not None else []
        self._need_f32_on(who, dev, list(operands) + mom)
        conv = self._trained_conv(who, layer, K.bn)
        named = dict(zip(K.order, operands))
        for j, (name, p) in enumerate(zip(K.params, self._params(kind, layer))):
            if tuple(named[name].shape) != tuple(p.shape) or any(t.numel() != p.numel() for t in [named["d." + name]] + mom[2 * j:2 * j + 2]):
                raise ValueError("Darknet.%s: layer %d takes %s, and gradients and moments of their sizes" % (who, layer, self._takes(K, conv)))
        _ffi.enqueue("rtod_plan_" + who, dev, self._plan, layer, C.byref(self._opt_step(opt)), *operands, *mom, *[None] * (n_mom - len(mom)))
        self._stepped[layer] = (kind, [named[name] for name in K.params])

    def _plan_is_current(self) -> bool:
        """A plan exists and holds the packed image of the parameters as they are (no re-pack is due at the next forward)."""
        batch_bn = bool(self.training and not self.bn_running_stats_in_train)
        return self._plan is not None and self._plan_weights_version == (self._weights_version, 0 if batch_bn else self._stats_version)

    def step_conv(self, layer: int, opt, weight, bias, dw, db, moments=None) -> None:
        """One optimiser step of a detection-head conv on the current stream (rtod_plan_step_conv): ``weight`` [Cout,Cin,1,1] and
        ``bias`` [Cout] are the caller's float32 device masters, updated IN PLACE from ``dw`` / ``db`` (``conv1x1_wgrad_async``)
        and, for Adam, ``moments = (exp_avg_w, exp_avg_sq_w, exp_avg_b, exp_avg_sq_b)``; the same kernel re-packs the conv's block
        of the plan's weight image in place.  ``opt``: an ``_ffi.OptStep`` or a mapping with its fields (kind 0 SGD / 1 Adam, lr,
        beta1, beta2, eps, step).  Nothing synchronises, nothing is allocated: legal under stream capture.  Needs a loaded plan
        that is current (a forward has run since the parameters last changed).  The module's ``conv.weight`` / ``conv.bias`` are
        NOT touched and lag behind from here on; ``weight_stream()``, ``state_dict()``, ``invalidate_weights()`` and every
        re-pack bring them up to date from these masters first (``sync_stepped_parameters``), reading ``conv.weight`` directly
        does not."""
        self._step("head", layer, opt, (weight, bias, dw, db), moments)

    def sync_stepped_parameters(self) -> None:
        """Copy the masters of every conv a step door has stepped into the module's parameters (``conv.weight`` / ``conv.bias``, for
        ``step_conv_bn`` ``bn.weight`` / ``bn.bias``; waits for the steps in flight).  The plan's image already holds them, so it
        stays valid: no re-pack follows."""
        if not self._stepped:
            return
        with torch.no_grad():
            for layer, (kind, masters) in self._stepped.items():
                for p, t in zip(self._params(kind, layer), masters):
                    p.copy_(t)
        self._stepped.clear()

    # ------------------------------------------------------------------ training under batch statistics (options keep_bn_inputs)
    def read_bn_input(self, layer: int, batch: int) -> torch.Tensor:
        """Dense NCHW copy of the raw conv output ``z`` that the last forward's BatchNorm step read for ``layer``
        (rtod_plan_read_bn_input): the ``z`` of ``train.bn_grad_async``.  Needs a model in ``.train()`` (batch statistics) with
        options ``keep_bn_inputs`` and a conv the plan trains under the keep option of the scope.  On a split-f16 plan (options
        ``bn_batch_split``) these are the fp32 sums the raw-sum conv instance wrote, the operand of that plan's normalise step."""
        if self._plan is None:
            raise RuntimeError("Darknet.read_bn_input: no plan yet; run a forward first")
        self._trained_conv("read_bn_input", layer, with_bn=True)
        c, h, w = C.c_int(), C.c_int(), C.c_int()                  # (z has the shape of the layer's own output)
        _ffi.check(_ffi.lib().rtod_plan_layer_shape(self._plan, int(layer), C.byref(c), C.byref(h), C.byref(w)))
        dev = torch.device("cuda", self._plan_key[2])
        out = torch.empty((int(batch), c.value, h.value, w.value), dtype=torch.float32, device=dev)
        _ffi.enqueue("rtod_plan_read_bn_input", dev, self._plan, int(layer), int(batch), out)
        return out

    def bn_stats_dev(self, layer: int):
        """``(mean address, var address)``: where the plan keeps the float64 mean and biased variance the last forward normalised
        ``layer`` with (rtod_plan_bn_stats_dev), in the style of ``conv_scale``; what ``train.bn_grad_async`` takes.  The
        addresses stay valid for the plan's life, every forward overwrites the values."""
        if not self._plan_is_current():
            raise RuntimeError("Darknet.bn_stats_dev: no loaded plan holds the current parameters; run a forward first")
        mean, var = C.c_void_p(), C.c_void_p()
        _ffi.check(_ffi.lib().rtod_plan_bn_stats_dev(self._plan, int(layer), C.byref(mean), C.byref(var)))
        return mean.value, var.value

    def step_conv_bn(self, layer: int, opt, weight, dw, gamma, beta, dgamma, dbeta, moments=None) -> None:
        """``step_conv_folded`` for a conv whose BatchNorm runs on batch statistics (rtod_plan_step_conv_bn): ``weight``
        [Cout,Cin,k,k], ``gamma`` and ``beta`` [Cout] are the caller's float32 device masters (``conv.weight``, ``bn.weight``,
        ``bn.bias``), updated IN PLACE from ``dw`` (``conv_wgrad_async`` of the ``dz`` of ``bn_grad_async``), ``dgamma`` and
        ``dbeta`` and, for Adam, ``moments = (exp_avg, exp_avg_sq)`` of the weight, of gamma, of beta: six tensors.  One kernel
        re-packs the unfolded conv and the [beta, gamma] block of the plan's image in place.  Nothing synchronises, nothing is
        allocated.  The module's parameters lag behind as after ``step_conv``."""
        self._step("bn", layer, opt, (weight, dw, gamma, beta, dgamma, dbeta), moments)

    def update_conv_bn(self, layer: int, weight, gamma, beta) -> None:
        """``update_conv_weight`` for a conv whose BatchNorm runs on batch statistics: ``weight`` [Cout,Cin,k,k], ``gamma`` and
        ``beta`` [Cout] go into ``conv.weight``, ``bn.weight`` and ``bn.bias`` and, when a plan with current weights is loaded,
        into that plan through rtod_plan_update_conv_bn, which re-packs this conv alone.  Synchronises."""
        self._update("bn", layer, (weight, gamma, beta))

    # ------------------------------------------------------------------ detection blocks (the BatchNorm conv a head conv reads)
    def _plan_list(self, who, entry, columns) -> list:
        """What ``head_blocks``, ``neck_layers`` and ``trainable_layers`` share: the plan's ``entry`` asked for its count, then for
        that many rows of ``columns`` ints."""
        if self._plan is None:
            raise RuntimeError("Darknet.%s: no plan yet; run a forward first" % who)
        n = entry(self._plan, *[None] * columns, 0)
        if n < 0:
            _ffi.check(n)
        arrays = [(C.c_int * max(n, 1))() for _ in range(columns)]
        entry(self._plan, *arrays, n)
        return list(zip(*[list(a)[:n] for a in arrays]))

    def head_blocks(self) -> list:
        """``[(head_conv_layer, block_conv_layer, block_input_layer)]`` per head in cfg order (rtod_plan_head_blocks): the block
        conv is the 1x1 / 3x3 stride-1 leaky or linear BatchNorm conv the head conv reads, where the plan can train it with
        BatchNorm frozen; ``(head, -1, -1)`` for a head without one.  ``read_layer(block_input_layer)`` is valid after a forward
        with options ``keep_block_inputs``.  Asks the plan, so a forward (or ``prepare``) must have run."""
        return self._plan_list("head_blocks", _ffi.lib().rtod_plan_head_blocks, 3)

    def neck_layers(self) -> list:
        """``[(neck_conv_layer, input_layer)]`` in ascending order (rtod_plan_neck_layers): the BatchNorm convs behind the backbone
        that the plan can train with the exact gradient of the loss, BatchNorm frozen — every reader of a neck layer is a neck
        layer or a [yolo] layer.  With options ``keep_neck_activations`` their inputs and outputs are valid ``read_layer`` targets
        after a forward and ``conv_scale`` / ``update_conv_weight`` / ``step_conv_folded`` accept each of them.  Asks the plan, so
        a forward (or ``prepare``) must have run."""
        return self._plan_list("neck_layers", _ffi.lib().rtod_plan_neck_layers, 2)

    def trainable_layers(self) -> list:
        """``[(conv_layer, input_layer)]`` in ascending order (rtod_plan_trainable_layers): the BatchNorm convs of the neck graph
        extended through 3x3 / stride-2 convs and ``[shortcut]`` layers — with options ``keep_backbone_activations`` every BatchNorm
        conv of YOLOv3 except layer 0; on YOLOv3-tiny the neck (its backbone is max-pools).  With that option their inputs and
        outputs are valid ``read_layer`` targets after a forward and ``conv_scale`` / ``update_conv_weight`` /
        ``step_conv_folded`` accept each of them.  Asks the plan, so a forward (or ``prepare``) must have run."""
        return self._plan_list("trainable_layers", _ffi.lib().rtod_plan_trainable_layers, 2)

    def full_layers(self) -> list:
        """``[(conv_layer, input_layer)]`` in ascending order (rtod_plan_full_layers): the BatchNorm convs of the trainable graph
        extended through convs of any ``Cin`` (layer 0 on a generic layout: ``input_layer`` -1, the network input) and size-2
        max-pools — with options ``keep_full_activations`` all 11 BatchNorm convs of YOLOv3-tiny (fp32); on YOLOv3 the trainable
        list, whose layer 0 runs the stem kernel.  With that option their inputs and outputs are valid ``read_layer`` targets after
        a forward and ``conv_scale`` / ``update_conv_weight`` / ``step_conv_folded`` accept each of them.  Asks the plan, so a
        forward (or ``prepare``) must have run."""
        return self._plan_list("full_layers", _ffi.lib().rtod_plan_full_layers, 2)

    def conv_scale(self, layer: int):
        """``(device address, host float64 array [Cout])`` of a block conv's frozen BatchNorm scale ``gamma / sqrt(var + 1e-5)`` as
        the plan folded it (rtod_plan_conv_scale); the address is what ``train.conv_wgrad_async(row_scale=...)`` takes and needs
        options ``keep_block_inputs`` (or ``keep_neck_activations`` / ``keep_backbone_activations``, under which any neck conv / any
        trainable conv is accepted)."""
        if not self._plan_is_current():
            raise RuntimeError("Darknet.conv_scale: no loaded plan holds the current parameters; run a forward first")
        conv = self._trained_conv("conv_scale", layer, with_bn=True)
        host = np.zeros(conv.out_channels, np.float64)
        dev = C.c_void_p()
        _ffi.check(_ffi.lib().rtod_plan_conv_scale(self._plan, int(layer), C.byref(dev), host, host.size))
        return dev.value, host

    def update_conv_weight(self, layer: int, weight) -> None:
        """``update_conv`` for a detection block conv, BatchNorm untouched: ``weight`` [Cout,Cin,k,k] goes into the module's
        ``conv.weight`` and, when a plan with current weights is loaded, into that plan through rtod_plan_update_conv_weight,
        which re-packs this conv alone (the bits a full re-pack gives).  Synchronises."""
        self._update("folded", layer, (weight,))

    def step_conv_folded(self, layer: int, opt, weight, dw, moments=None) -> None:
        """``step_conv`` for a detection block conv (rtod_plan_step_conv_folded): ``weight`` [Cout,Cin,k,k] is the caller's RAW
        float32 device master (the module's ``conv.weight``, not the folded one), updated IN PLACE from ``dw``
        (``conv_wgrad_async`` with the plan's scale) and, for Adam, ``moments = (exp_avg, exp_avg_sq)``; the same kernel folds the
        frozen BatchNorm scale and re-packs the conv's block of the plan's weight image in place.  Nothing synchronises, nothing
        is allocated.  Needs a current plan with options ``keep_block_inputs``, ``keep_neck_activations`` or ``keep_backbone_activations``
        (the widest of them decides which convs are accepted).  ``conv.weight`` lags behind as after ``step_conv``."""
        self._step("folded", layer, opt, (weight, dw), moments)

    def packed_weights(self) -> np.ndarray:
        """The plan's packed weight image as it is on the device now, as uint32 words (rtod_plan_read_packed_weights; tests and
        debugging; synchronises)."""
        if self._plan is None:
            raise RuntimeError("Darknet.packed_weights: no plan yet; run a forward first")
        need = C.c_size_t()
        _ffi.check(_ffi.lib().rtod_plan_read_packed_weights(self._plan, None, 0, C.byref(need)))
        out = np.zeros(need.value, np.float32)
        with torch.cuda.device(self._plan_key[2]):
            _ffi.check(_ffi.lib().rtod_plan_read_packed_weights(self._plan, out, out.size, None))
        return out.view(np.uint32)

    # ------------------------------------------------------------------ plan
    def _destroy_plan(self):
        if self._plan is not None:
            _ffi.lib().rtod_plan_destroy(self._plan)
            self._plan = None
            self._plan_key = None

    def __del__(self):
        try:
            self._destroy_plan()
        except Exception:
            pass

    def prepare(self, max_batch: int, device=None):
        """Build the native plan for ``net_info['height']`` and ``max_batch`` frames and upload the
        BN-folded, K-major packed weights.  Called lazily by ``forward``."""
        lib = _ffi.lib()
        if device is None:
            device = torch.cuda.current_device()
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        inp_dim = int(self.net_info["height"])
        width = inp_dim if self.input_width is None else int(self.input_width)
        if self.precision not in ("fp32", "f16s3", "f16", "auto"):
            raise ValueError("Darknet.precision must be 'fp32', 'f16s3', 'f16' or 'auto'")
        # BatchNorm semantics follow the module's mode like nn.BatchNorm2d: eval() = running statistics, folded into the convs
        # (the fast path, frame-independent); training mode = the statistics of the batch — what the reference's callers
        # actually run, since they never call .eval() (detect.py:185-194).  That mode is a parity path on the
        # exact-fp32 kernels (conv -> per-channel statistics -> normalise), several times slower and batch-dependent.
        # options = {"bn_batch_split": 1} (opt-in) runs that mode on the split-f16 kernels where the cfg allows it: raw-sum conv
        # instances, the same statistics kernels, a normalise kernel that writes the split format (precision "f16s3" / "auto").
        batch_bn = bool(self.training and not self.bn_running_stats_in_train)
        bn_split = bool(batch_bn and int(self.options.get("bn_batch_split", 0)))
        if batch_bn and (self.precision == "f16" or (self.precision == "f16s3" and not bn_split)):
            raise RuntimeError("Darknet is in training mode (batch-statistics BatchNorm, like the reference without .eval()): that "
                               "path runs on the exact-fp32 kernels only; call .eval() for the %s kernels or set precision='auto'"
                               % ("split-f16" if self.precision == "f16s3" else "plain-f16"))
        if batch_bn and self.input_width is not None and width != inp_dim:
            raise RuntimeError("Darknet is in training mode (batch-statistics BatchNorm, the reference's square path): a rectangular "
                               "input (input_width=%d, height %d) runs in eval mode only; call .eval()" % (width, inp_dim))
        if batch_bn and not self._warned_batch_bn:
            warnings.warn("Darknet is in training mode: BatchNorm uses the statistics of the batch, as the reference does when its "
                          "callers skip .eval() (slow parity path, results depend on the batch); call .eval() for the fast, "
                          "frame-independent path", RuntimeWarning)
            self._warned_batch_bn = True
        opts = dict(self.options)
        if batch_bn:
            opts["bn_batch_stats"] = 1
        key = (inp_dim, int(max_batch), device.index, bool(self.keep_all_layers), "fp32" if batch_bn and not bn_split else self.precision, tuple(sorted(opts.items())),
               self.input_width is not None, width)
        if self._plan is None or self._plan_key != key:
            self._destroy_plan()
            h = C.c_void_p()
            txt = self._cfg_text.encode()
            if self.input_width is None:
                _ffi.check(lib.rtod_plan_create(txt, len(txt), inp_dim, inp_dim, int(max_batch), device.index, C.byref(h)))
            else:
                _ffi.check(lib.rtod_plan_create_rect(txt, len(txt), inp_dim, width, int(max_batch), device.index, C.byref(h)))
            self._plan, self._plan_key = h, key
            self._tuned = set()
            if self.keep_all_layers:
                _ffi.check(lib.rtod_plan_set_keep_all_layers(self._plan, 1))
            for name, value in sorted(opts.items()):
                _ffi.check(lib.rtod_plan_set_option(self._plan, name.encode(), int(value)))
            if self._ovf is None or self._ovf.device != device:
                self._ovf = torch.zeros(1, dtype=torch.int32, device=device)
            _ffi.check(lib.rtod_plan_set_overflow_flag(self._plan, self._ovf))
            # "auto": the split-f16 kernels when the cfg supports them (yolov3 does; a cfg with a conv after layer 0 whose
            # Cin % 32 != 0 does not — yolov3-tiny's 16-channel layer 2 does with options = {"narrow_cin": 1}, already set
            # above), else the exact-fp32 MFMA kernels.  Both are HIP paths.
            if self.precision == "fp32" or (batch_bn and not bn_split):
                self.active_precision = "fp32"
            elif self.precision == "f16":                        # opt-in only: "auto" never picks it
                _ffi.check(lib.rtod_plan_set_precision(self._plan, 2))
                self.active_precision = "f16"
            else:
                rc = lib.rtod_plan_set_precision(self._plan, 1)
                if rc == 0:
                    self.active_precision = "f16s3"
                elif self.precision == "auto" and rc == -3:
                    self.active_precision = "fp32"
                else:
                    _ffi.check(rc)
            if self.active_precision == "fp32":
                _ffi.check(lib.rtod_plan_set_precision(self._plan, 0))
            self._plan_weights_version = -1
            info = _ffi.PlanInfo()
            _ffi.check(lib.rtod_plan_get_info(self._plan, C.byref(info)))
            self._info = info
        version = (self._weights_version, 0 if batch_bn else self._stats_version)
        if self._plan_weights_version != version:
            w = np.ascontiguousarray(self.weight_stream())
            with torch.cuda.device(device):
                _ffi.check(lib.rtod_plan_load_weights(self._plan, w, w.size))
            self._plan_weights_version = version
        return self._info

    # ------------------------------------------------------------------ tile tables (autotune results)
    def get_tiles(self, batch: int) -> list:
        """Tile variant per launch that autotune chose for this batch size (rtod_plan_get_tiles)."""
        lib = _ffi.lib()
        n = lib.rtod_plan_get_tiles(self._plan, int(batch), None, 0)
        if n < 0:
            _ffi.check(n)
        arr = (C.c_int * n)()
        got = lib.rtod_plan_get_tiles(self._plan, int(batch), arr, n)
        if got < 0:
            _ffi.check(got)
        return list(arr)

    def set_tiles(self, batch: int, variants) -> None:
        """Install a tile table (e.g. saved by another process) for this batch size: forwards of that size then launch exactly
        those kernels and measure nothing.  The plan must exist (prepare / a forward at a larger or equal batch size)."""
        arr = (C.c_int * len(variants))(*[int(v) for v in variants])
        _ffi.check(_ffi.lib().rtod_plan_set_tiles(self._plan, int(batch), arr, len(variants)))
        self._tuned.add(int(batch))

    def plan_description(self) -> dict:
        lib = _ffi.lib()
        need = C.c_size_t()
        _ffi.check(lib.rtod_plan_describe(self._plan, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _ffi.check(lib.rtod_plan_describe(self._plan, buf, need.value, None))
        return json.loads(buf.value.decode())

    def launch_infos(self):
        lib = _ffi.lib()
        out = []
        for i in range(self._info.n_launches):
            li = _ffi.LaunchInfo()
            _ffi.check(lib.rtod_plan_get_launch(self._plan, i, C.byref(li)))
            out.append(li)
        return out

    # ------------------------------------------------------------------ forward
    def _check_input(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("Darknet.forward: input must be a CUDA (ROCm) tensor; this build has no CPU path")
        if x.dtype != torch.float32 or x.dim() != 4 or x.size(1) != 3:
            raise ValueError("Darknet.forward: expected float32 [B,3,H,W], got %s %s" % (x.dtype, tuple(x.shape)))
        inp_dim = int(self.net_info["height"])
        if self.input_width is not None:
            if x.size(2) != inp_dim or x.size(3) != int(self.input_width):
                raise ValueError("Darknet.forward: input is %dx%d (HxW) but the model expects net_info['height'] x input_width = %dx%d"
                                 % (x.size(2), x.size(3), inp_dim, int(self.input_width)))
            return inp_dim
        if x.size(2) != inp_dim or x.size(3) != inp_dim:
            raise ValueError("Darknet.forward: input is %dx%d but net_info['height'] = %d (set it like detect.py:47 does)"
                             % (x.size(2), x.size(3), inp_dim))
        return inp_dim

    def forward(self, x, _launch_ms=None):
        self._check_input(x)
        lib = _ffi.lib()
        B = x.size(0)
        max_batch = B if self._plan_key is None else max(B, self._plan_key[1])
        info = self.prepare(max_batch, x.device)
        x = x.contiguous()
        out = torch.empty((B, info.total_rows, info.attrs), dtype=torch.float32, device=x.device)
        _ffi.check(lib.rtod_plan_set_train_decode(self._plan, 1 if self.TRAIN else 0))      # (host state of the plan)
        if _launch_ms is not None:
            _ffi.enqueue("rtod_forward_timed", x.device, self._plan, x, B, out, after=(_launch_ms,))
        elif self.autotune and self.active_precision in ("f16s3", "f16") and B not in self._tuned:
            # first forward of a batch size: measures the tile variants (synchronises); rtod_forward itself never does
            _ffi.enqueue("rtod_plan_autotune", x.device, self._plan, x, B, out)
            self._tuned.add(B)
        else:
            _ffi.enqueue("rtod_forward", x.device, self._plan, x, B, out)
        if self.training and not self.bn_running_stats_in_train and self.update_running_stats and _launch_ms is None:
            self._update_running_stats(B)
        # attributes the reference sets as a side effect of forward (src/darknet.py:239-243, 260)
        anchors = []
        for m, blk in zip(self.module_list, self.blocks[1:]):
            if blk["type"] == "yolo":
                anchors.extend(m[0].anchors)
                self.num_classes = int(blk["classes"])
        self.anchors = anchors
        if self.active_precision in ("f16s3", "f16") and self.overflow_check != "off":
            if self.overflow_check == "forward":
                if self.overflowed():
                    if self.precision != "auto":
                        raise FloatingPointError(_OVERFLOW_MSG)
                    warnings.warn("Darknet: an activation left the split-f16 range (|x| >= 8188); precision 'auto' falls back to the "
                                  "exact-fp32 MFMA kernels for this model", RuntimeWarning)
                    self.precision = "fp32"
                    return self.forward(x)
            else:
                self._forward_seq += 1
                out._rtod_forward = (weakref.ref(self), self._forward_seq)
        return out

    def _update_running_stats(self, batch):
        """Training-mode side effect of nn.BatchNorm2d (momentum 0.1): running_mean / running_var move towards the batch's mean
        and UNBIASED variance, num_batches_tracked counts up — the reference mutates them on every forward.
        One kernel launch for all BatchNorm layers (rtod_plan_bn_update_running), no host round trip: the module buffers are
        updated in place on the device, behind the forward on the same stream."""
        bns = [sub for m in self.module_list for sub in m.children() if isinstance(sub, nn.BatchNorm2d)]
        if not bns:
            return
        dev = torch.device("cuda", self._plan_key[2])
        mom = {bn.momentum if bn.momentum is not None else 0.1 for bn in bns}
        if len(mom) != 1:
            raise RuntimeError("Darknet: BatchNorm layers with different momenta are not supported")
        for bn in bns:                                             # the buffers live where the plan runs (the reference: model.cuda())
            for name in ("running_mean", "running_var", "num_batches_tracked"):
                t = getattr(bn, name)
                if t.device != dev:
                    setattr(bn, name, t.to(dev))
            if bn.running_mean.dtype != torch.float32 or not bn.running_mean.is_contiguous() or not bn.running_var.is_contiguous():
                raise RuntimeError("Darknet: BatchNorm running statistics must be contiguous float32 tensors")
        n = len(bns)
        rm = (C.c_void_p * n)(*[bn.running_mean.data_ptr() for bn in bns])
        rv = (C.c_void_p * n)(*[bn.running_var.data_ptr() for bn in bns])
        _ffi.enqueue("rtod_plan_bn_update_running", dev, self._plan, int(batch), rm, rv, n, float(mom.pop()))
        with torch.cuda.device(dev):
            torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        self._stats_version += 1                # an eval-mode plan built later folds the updated statistics

    def overflowed(self) -> bool:
        """True when a split-f16 producer saturated since the last call (one small host sync); clears the flag."""
        if self._ovf is None:
            return False
        hit = bool(int(self._ovf.item()))
        if hit:
            self._ovf.zero_()
        return hit

    def check_overflow(self):
        if self.overflowed():
            raise FloatingPointError(_OVERFLOW_MSG)

    def make_graphed(self, example_x, post=None):
        """Capture ``forward`` (and optionally ``post(y)``, e.g. ``util.write_results_async``) for ``example_x``'s shape into a
        HIP graph and return ``run(x) -> (y, post result)``.  ``rtod_forward`` only enqueues, so the whole launch list replays
        as one graph launch: for small batches (YOLOv3-tiny batch 1: 24 launches of a few microseconds each) the per-launch
        host cost is what limits the latency.  ``run`` copies ``x`` into a static input buffer and returns the static output
        tensors: consume or clone them before the next call.  The range flag of split-f16 plans is not read (use
        ``overflowed()``)."""
        self._check_input(example_x)
        dev = example_x.device
        static_x = example_x.clone()
        keep = self.overflow_check
        self.overflow_check = "off"
        try:
            with torch.no_grad():
                y = self.forward(static_x)                                # builds the plan, autotunes this batch size
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):                             # warm-up on a non-default stream, as capture requires
                    y = self.forward(static_x)
                    r = post(y) if post is not None else None
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    y = self.forward(static_x)
                    r = post(y) if post is not None else None
        finally:
            self.overflow_check = keep

        def run(x):
            static_x.copy_(x, non_blocking=True)
            graph.replay()
            return y, r
        run.graph = graph
        return run

    def forward_timed(self, x):
        """Forward with a HIP-event pair around every launch; returns (out, ms per launch)."""
        self._check_input(x)
        info = self.prepare(x.size(0) if self._plan_key is None else max(x.size(0), self._plan_key[1]), x.device)
        ms = (C.c_float * info.n_launches)()
        out = self.forward(x, _launch_ms=ms)
        return out, np.frombuffer(ms, dtype=np.float32).copy()

    def read_layer(self, layer: int, batch: int) -> torch.Tensor:
        """Dense NCHW copy of a materialised layer output of the last forward (tests/debug)."""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        _ffi.check(_ffi.lib().rtod_plan_layer_shape(self._plan, layer, C.byref(c), C.byref(h), C.byref(w)))
        dev = torch.device("cuda", self._plan_key[2])
        out = torch.empty((batch, c.value, h.value, w.value), dtype=torch.float32, device=dev)
        _ffi.enqueue("rtod_plan_read_layer", dev, self._plan, layer, batch, out)
        return out

    @contextmanager
    def train_mode(self):
        """Decode without grid offsets / anchors (reference: src/darknet.py:305-314)."""
        try:
            self.TRAIN = True
            yield
        finally:
            self.TRAIN = False

    def finish_decode(self, prediction):
        """Turn the output of a forward run under ``train_mode()`` into the eval decode, in place (rtod_plan_finish_decode): the
        tensor is then bit-identical to ``forward`` of the same input outside ``train_mode()``, so one forward serves the loss
        and the detections.  Uses the plan of the last forward; returns ``prediction``."""
        if self._plan is None or self._info is None:
            raise RuntimeError("Darknet.finish_decode: no forward has run yet")
        p = prediction
        if not isinstance(p, torch.Tensor) or not p.is_cuda:
            raise RuntimeError("Darknet.finish_decode: expected a CUDA (ROCm) tensor; this build has no CPU path")
        if p.dtype != torch.float32 or p.dim() != 3 or not p.is_contiguous() or tuple(p.shape[1:]) != (self._info.total_rows, self._info.attrs):
            raise ValueError("Darknet.finish_decode: expected the contiguous float32 [B,%d,%d] output of forward, got %s %s"
                             % (self._info.total_rows, self._info.attrs, p.dtype, tuple(p.shape)))
        _ffi.enqueue("rtod_plan_finish_decode", p.device, self._plan, p, p.size(0))
        return p
