"""Host-side mirror of the loss side of the reference's trainer (``DarknetTrainer``, train.py:17-230) on librtod.so.

The FORWARD VALUE of the loss: targets from ground-truth boxes (``target_creator``) and the five-term sum of squares
(``darknet_loss``), the last step of ``feed_forward_through_model`` (train.py:412-425); and the first layer of its backward pass:
the gradient with respect to the raw head maps and from it ``dW``, ``db`` of the detection-head convs (the 1x1 convs without
BatchNorm in front of the [yolo] blocks), with a plain SGD step on them — fine-tuning the heads with the backbone frozen — and, with
``trainable="blocks"``, one layer further: the weight gradient of the BatchNorm conv each head conv reads, BatchNorm frozen, with
``trainable="neck"`` every BatchNorm conv behind the backbone, and with ``trainable="backbone"`` the backbone too: every BatchNorm conv
the plan can train (``Darknet.trainable_layers``: on YOLOv3 all but layer 0), through 3x3 / stride-2 convs and residual shortcuts,
and with ``trainable="full"`` through size-2 max-pools, convs of any Cin and a generic-layout layer 0 too (``Darknet.full_layers``: all
11 BatchNorm convs of YOLOv3-tiny).
On a model left in ``.train()`` with ``options['keep_bn_inputs']`` (batch mode: exact fp32, or precision "f16s3" with
``options['bn_batch_split']``, where the forward runs the split-f16 raw-sum kernels and the backward stays exact fp32 over the values that
forward stored) every scope trains under the statistics of the batch, as the reference's trainer does: the walk goes through the BatchNorm backward (``bn_grad_async``) and ``bn.weight`` and
``bn.bias`` are stepped beside the conv weights (``batchnorm_gradients``).  Symmetric-pool and SiLU backward, weight decay, epochs and
data loaders are out of scope.  The reference's
optimiser — ``optim.Adam(lr=1e-2)``, train.py:57 — runs on the trained convs as one kernel per conv that also re-packs the conv's weights in
place (``HeadOptimizer``, ``feed_forward_through_model``): that path never synchronises.  Same names and return conventions as the
reference:

* ``DarknetTrainer.anchor_fit(box, anchors)``, ``target_layer(bboxes, scale, anchors)``     host mirrors, train.py:167-209
* ``DarknetTrainer.target_creator(bndbox) -> (target, mask)``                               train.py:129-149, one launch sequence
* ``DarknetTrainer.darknet_loss(pred, target, obj_mask)`` (``criterion``)                   train.py:211-230, dense tensors
* ``DarknetTrainer.loss_from_boxes(pred, bndbox) -> (loss, components)``                    both fused: no dense target is built
* ``DarknetTrainer.forward_loss(frames_or_x, bndbox)``                                      forward under ``train_mode()`` + loss
* ``DarknetTrainer.head_gradients(frames_or_x, bndbox) -> (loss, {conv_layer: (dW, db)})``  (new) what ``loss.backward()`` leaves on the heads
* ``DarknetTrainer.head_step(frames_or_x, bndbox, lr)``                                     (new) ``w -= lr * dW``, ``b -= lr * db`` on the heads
* ``DarknetTrainer.feed_forward_through_model(batch_data, bndbox)``                         train.py:412-425: forward, loss, backward, ``optimizer`` step
* ``DarknetTrainer.optimizer`` (``HeadOptimizer``: Adam or SGD on the heads), ``sync_parameters()``    train.py:57
* ``DarknetTrainer.gradients(frames_or_x, bndbox, scope=None)``                             (new) ``(loss, head grads, {conv_layer: dW})`` behind the heads: ONE walk
                                                                                            (``_walk``) over the graph of ``scope`` (``_graph``); the three entries
                                                                                            below are ``gradients`` with their scope
* ``DarknetTrainer(model, trainable="blocks")``, ``block_gradients(frames_or_x, bndbox)``             (new) the step also trains the conv in front of
                                                                                            each head conv: ``(loss, head grads, {block_conv_layer: dW})``
* ``DarknetTrainer(model, trainable="neck")``, ``neck_gradients(frames_or_x, bndbox)``                (new) ... and every BatchNorm conv behind the
                                                                                            backbone (``Darknet.neck_layers``), through 3x3 convs, routes and the
                                                                                            upsample: ``(loss, head grads, {neck_conv_layer: dW})``
* ``DarknetTrainer(model, trainable="backbone")``, ``backbone_gradients(frames_or_x, bndbox)``        (new) ... and the backbone (``Darknet.trainable_layers``),
                                                                                            through stride-2 convs (``conv_dgrad_async`` / ``conv_wgrad_async``
                                                                                            with ``stride=2``) and shortcuts, fan-out sums by ``grad_join_async``
* ``DarknetTrainer(model, trainable="full")``, ``full_gradients(frames_or_x, bndbox)``                (new) ... and YOLOv3-tiny's backbone (``Darknet.full_layers``):
                                                                                            max-pools (``maxpool_grad_async``), thin convs
                                                                                            (``conv_wgrad_thin_async`` / ``conv_dgrad_thin_async``) and layer 0

* ``bn_grad_async(du, z, mean, var, gamma) -> (dz, dgamma, dbeta)``, ``bn_grad_parts(batch, channels, pixels)``   (new) rtod_bn_grad: the backward of
                                                                                            batch-statistics BatchNorm, double sums over a fixed partition
* ``DarknetTrainer.batchnorm_gradients(frames_or_x, bndbox, scope=None)``                   (new) ``gradients`` with ``{conv_layer: (dgamma, dbeta)}`` as a
                                                                                            fourth element; in batch mode ``feed_forward_through_model`` steps
                                                                                            conv weight, gamma and beta (``Darknet.step_conv_bn``)

The reference's behaviour is kept as it is: only boxes whose class-0 slot is 1 and whose sides are at least
``min_box_size`` (24) count, ``anchor_fit`` compares a box with a square of the anchor's WIDTH, target slot 0 holds the y fraction
and slot 1 the x fraction, the later of two boxes on one (cell, anchor) wins.  Heads come from the model's cfg (grid = input /
stride, anchors by mask, cfg order) instead of the reference's hard-coded 13 / 26 / 52; at 416 the two agree.  A box whose cell lies
outside a head's grid is skipped there and sets bit 0 of ``status``.  Loss kernels need CUDA (ROCm) tensors; no CPU fallback.
"""
import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _ffi
from .cfg import build_ir
from .darknet import CONV_KINDS
from .util import _need_cuda, prep_frames


def _workspace(dev, batch, n_rows):
    return _ffi.workspace("rtod_yolo_loss", dev, batch, n_rows)


def make_heads(heads):
    """ctypes array of rtod_yolo_head from ``[(grid_h, grid_w, stride, [(w, h), ...]), ...]``."""
    arr = (_ffi.YoloHead * max(len(heads), 1))()
    for q, (gh, gw, stride, anchors) in zip(arr, heads):
        if len(anchors) > 8:
            raise ValueError("yolo_loss: a head has %d anchors, the kernel takes at most 8" % len(anchors))
        q.grid_h, q.grid_w, q.stride, q.n_anchors = int(gh), int(gw), int(stride), len(anchors)
        for a, (w, h) in enumerate(anchors):
            q.anchors[2 * a], q.anchors[2 * a + 1] = int(w), int(h)
    return arr


def pack_boxes(bndbox, attrs, dev):
    """Per-image box lists -> (boxes [sum T, attrs] float32, offsets int32 [B+1]) on ``dev``; nothing synchronises."""
    offs, parts = [0], []
    for t in bndbox:
        t = None if t is None or isinstance(t, int) else torch.as_tensor(t, dtype=torch.float32)
        n = 0
        if t is not None and t.numel():
            parts.append(t.reshape(-1, attrs))
            n = parts[-1].size(0)
        offs.append(offs[-1] + n)
    if parts and all(p.is_cuda for p in parts):
        boxes = torch.cat(parts).contiguous()
    elif parts:
        boxes = torch.cat([p.cpu() for p in parts]).contiguous().pin_memory().to(dev, non_blocking=True)
    else:
        boxes = torch.zeros((1, attrs), dtype=torch.float32, device=dev)
    return boxes, torch.tensor(offs, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)


def _loss_prelude(who, pred, bndbox, num_class, status):
    """What ``yolo_loss_async`` and ``yolo_loss_grad_async`` do before their launch: the checks of ``pred`` and ``bndbox``, the
    packed boxes, the workspace, and the outputs both have.  Returns ``(B, N, attrs, dev, boxes, offsets, (workspace, bytes), out)``."""
    _need_cuda(pred, who)
    attrs = 5 + int(num_class)
    if pred.dim() != 3 or pred.size(2) != attrs or not pred.is_contiguous():
        raise ValueError("%s: expected contiguous predictions [B,N,%d], got %s" % (who, attrs, tuple(pred.shape)))
    B, N = pred.size(0), pred.size(1)
    if len(bndbox) != B:
        raise ValueError("%s: %d box lists for a batch of %d" % (who, len(bndbox), B))
    dev = pred.device
    boxes, offs = pack_boxes(bndbox, attrs, dev)
    out = {"components": torch.empty(6, dtype=torch.float64, device=dev), "n_obj": torch.empty(B, dtype=torch.int32, device=dev),
           "status": status if status is not None else torch.zeros(1, dtype=torch.int32, device=dev)}
    return B, N, attrs, dev, boxes, offs, _workspace(dev, B, N), out


def yolo_loss_async(pred, bndbox, heads, num_class, min_box_size=24, dense=False, per_image=False, status=None):
    """Enqueue rtod_yolo_loss for one batch; nothing synchronises.  ``pred`` [B,N,5+C] (TRAIN=True decode), ``bndbox`` one
    ``[T_i, 5+C]`` tensor (or None / empty) per image, ``heads`` as for ``make_heads``.  Returns a dict of device tensors:
    ``components`` float64 [6] (total, xy, wh, obj, noobj, cls), ``n_obj`` int32 [B], ``status`` int32 [1] (OR-ed into the caller's
    if given), and with ``per_image`` float64 [B,6], with ``dense`` ``target`` float32 [B,N,5+C] and ``mask`` uint8 [B,N]."""
    B, N, attrs, dev, boxes, offs, (ws, nbytes), out = _loss_prelude("yolo_loss", pred, bndbox, num_class, status)
    if per_image:
        out["per_image"] = torch.empty((B, 6), dtype=torch.float64, device=dev)
    if dense:
        out["target"] = torch.empty((B, N, attrs), dtype=torch.float32, device=dev)
        out["mask"] = torch.empty((B, N), dtype=torch.uint8, device=dev)
    _ffi.enqueue("rtod_yolo_loss", dev, pred, B, N, int(num_class), make_heads(heads), len(heads), boxes, offs, float(min_box_size),
                 out["components"], out.get("per_image"), out.get("target"), out.get("mask"), out["n_obj"], out["status"], ws, nbytes)
    return out


def yolo_loss_grad_async(pred, bndbox, heads, num_class, min_box_size=24, grad_pred=False, status=None):
    """Enqueue rtod_yolo_loss_grad for one batch; nothing synchronises.  Arguments as ``yolo_loss_async``.  Returns a dict of
    device tensors: ``grad_raw`` a list with one ``[B, A*attrs, GH, GW]`` view per head (the gradient with respect to the raw head
    maps, views of one buffer ``grad_raw_flat``), ``components`` float64 [6] (bit-identical to ``yolo_loss_async``), ``n_obj``,
    ``status``, and with ``grad_pred`` the gradient with respect to ``pred`` [B,N,5+C]."""
    B, N, attrs, dev, boxes, offs, (ws, nbytes), out = _loss_prelude("yolo_loss_grad", pred, bndbox, num_class, status)
    out["grad_raw_flat"] = torch.empty(B * N * attrs, dtype=torch.float32, device=dev)
    if grad_pred:
        out["grad_pred"] = torch.empty((B, N, attrs), dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_yolo_loss_grad", dev, pred, B, N, int(num_class), make_heads(heads), len(heads), boxes, offs, float(min_box_size),
                 out["grad_raw_flat"], out.get("grad_pred"), out["components"], out["n_obj"], out["status"], ws, nbytes)
    views, off = [], 0
    for gh, gw, _, anchors in heads:                                  # head h at float offset B * sum of the earlier heads' A * attrs * GH * GW
        n = B * len(anchors) * attrs * gh * gw
        views.append(out["grad_raw_flat"][off:off + n].view(B, len(anchors) * attrs, gh, gw))
        off += n
    out["grad_raw"] = views
    return out


# (no size, stride, thin) -> the C entry of _wgrad (its workspace entry: the name + "_workspace"), whether it takes a row scale, a db
_WGRAD_ENTRIES = {(True, 1, False): ("rtod_conv1x1_wgrad", False, True), (False, 1, False): ("rtod_conv_wgrad", True, True),
                  (False, 2, False): ("rtod_conv_wgrad_s2", True, True), (False, 1, True): ("rtod_conv_wgrad_thin", True, False)}
_DGRAD_ENTRIES = {(True, 1, False): "rtod_conv1x1_dgrad", (False, 1, False): "rtod_conv_dgrad", (False, 2, False): "rtod_conv_dgrad_s2",
                  (False, 1, True): "rtod_conv_dgrad_thin"}                 # ... of _dgrad; every entry with a size takes a row scale


def _wgrad(who, dz, x, size, row_scale, bias, stride=1, thin=False):
    """The body of ``conv1x1_wgrad_async`` (``size`` None: rtod_conv1x1_wgrad, shape (B, Cout, Cin, pixels)) and ``conv_wgrad_async``
    (rtod_conv_wgrad, shape (B, Cout, Cin, H, W, size); ``stride`` 2: rtod_conv_wgrad_s2, H x W the map of ``x``): the tensor checks, the
    workspace cached per shape, the outputs, the launch.  ``thin``: rtod_conv_wgrad_thin (any Cin, stride 1, no ``db``)."""
    _need_cuda(dz, who)
    _need_cuda(x, who)
    if stride not in (1, 2) or (stride == 2 and size is None):
        raise ValueError("%s: stride must be 1 or 2, got %r" % (who, stride))
    s2 = stride == 2
    ok = dz.dim() == 4 and x.dim() == 4 and dz.size(0) == x.size(0) and dz.dtype == torch.float32 and x.dtype == torch.float32
    if ok:
        ok = tuple(dz.shape[2:]) == (tuple((n - 1) // 2 + 1 for n in x.shape[2:]) if s2 else tuple(x.shape[2:]))
    if not ok:
        raise ValueError("%s: expected float32 dz [B,Cout,%s] and x [B,Cin,H,W], got %s and %s" % (who, "(H-1)//2+1,(W-1)//2+1" if s2 else "H,W", tuple(dz.shape), tuple(x.shape)))
    dz, x = dz.contiguous(), x.contiguous()
    B, cout, cin, H, W = dz.size(0), dz.size(1), x.size(1), x.size(2), x.size(3)
    shape = (B, cout, cin, H * W) if size is None else (B, cout, cin, H, W, int(size))
    dev = dz.device
    name, takes_scale, takes_db = _WGRAD_ENTRIES.get((size is None, stride, bool(thin)), (None, False, False))
    if thin and (name is None or bias):
        raise ValueError("%s: the thin entry takes a size, stride 1 and no bias gradient" % who)
    scale = (_scale_ptr(row_scale, cout, dev),) if takes_scale else ()
    k = 1 if size is None else int(size)
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=dev)
    db = torch.empty(cout, dtype=torch.float32, device=dev) if bias else None
    _ffi.enqueue(name, dev, dz, x, *shape, *scale, dw, *((db,) if takes_db else ()), *_ffi.workspace(name, dev, *shape))
    return dw, db


def conv1x1_wgrad_async(dz, x, bias=True):
    """Enqueue rtod_conv1x1_wgrad: ``dz`` [B,Cout,H,W] and ``x`` [B,Cin,H,W] (contiguous float32 device tensors, Cin a multiple
    of 32) -> ``(dW [Cout,Cin,1,1], db [Cout] or None)``; nothing synchronises."""
    return _wgrad("conv1x1_wgrad", dz, x, None, None, bias)


def _scale_ptr(row_scale, cout, dev):
    """``row_scale`` of ``conv_wgrad_async`` as a pointer argument: None, a float64 device tensor [Cout] (checked), or an integer
    device address (what ``Darknet.conv_scale`` hands out)."""
    if isinstance(row_scale, torch.Tensor):
        if row_scale.device != dev or row_scale.dtype != torch.float64 or row_scale.numel() != cout or not row_scale.is_contiguous():
            raise ValueError("conv_wgrad: row_scale must be a contiguous float64 tensor [%d] on %s" % (cout, dev))
        return row_scale
    return None if row_scale is None else int(row_scale)


def conv_wgrad_async(dz, x, size, row_scale=None, bias=False, stride=1):
    """Enqueue rtod_conv_wgrad: ``dz`` [B,Cout,H,W] and ``x`` [B,Cin,H,W] (contiguous float32 device tensors, Cin a multiple of
    32) -> ``(dW [Cout,Cin,size,size], db [Cout] or None)`` of a ``size`` x ``size`` (1 or 3), stride-1, same-padding conv.
    ``row_scale`` (float64 device tensor [Cout], or the device address ``Darknet.conv_scale`` returns): every row of dW times it,
    one rounding.  ``stride`` 2 (rtod_conv_wgrad_s2): a 3x3 / stride-2 / pad-1 conv, ``dz`` [B,Cout,(H-1)//2+1,(W-1)//2+1] on the
    conv's output map.  A ``Cin`` that is no multiple of 32 goes to the entry of ``conv_wgrad_thin_async`` (stride 1, no ``db``), and
    only such a one.  Nothing synchronises; the workspace is cached per shape."""
    thin = isinstance(x, torch.Tensor) and x.dim() == 4 and x.size(1) % 32 != 0
    return _wgrad("conv_wgrad_thin" if thin else "conv_wgrad", dz, x, int(size), row_scale, bias, stride, thin)


def conv_wgrad_thin_async(dz, x, size, row_scale=None, bias=False, stride=1):
    """Enqueue rtod_conv_wgrad_thin: ``conv_wgrad_async`` for a 1x1 or 3x3 / stride-1 conv of ANY ``Cin`` (YOLOv3-tiny's layers 0
    and 2: few channels, a huge K) -> ``dW [Cout,Cin,size,size]``.  A 32 x 128 tile, the slice count cut for K
    (``conv_wgrad_thin_slices``), the slice sums added as a fixed two-level tree; no ``db`` (these are BatchNorm convs)."""
    return _wgrad("conv_wgrad_thin", dz, x, int(size), row_scale, bias, stride, thin=True)[0]


def conv_wgrad_thin_slices(batch, cout, cin, height, width, size):
    """``(slices, slice_len)`` of rtod_conv_wgrad_thin for that shape (rtod_conv_wgrad_thin_slices): no fmaf chain is longer than
    ``slice_len`` terms, and ``slices`` partial sums are added per element."""
    s, n = C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().rtod_conv_wgrad_thin_slices(int(batch), int(cout), int(cin), int(height), int(width), int(size), C.byref(s), C.byref(n)))
    return s.value, n.value


def _dgrad_operands(who, w, dz, size, y, stride=1, in_hw=None):
    """The operand check ``_dgrad`` and ``conv_dgrad_split_async`` share.  Returns ``(w, dz, y)`` contiguous and ``(H, W)``, the map
    ``dx`` lives on (for ``stride`` 2 the conv's INPUT map, from ``y`` or ``in_hw``)."""
    for t in (w, dz) + ((y,) if y is not None else ()):
        _need_cuda(t, who)
    k = 1 if size is None else int(size)
    if stride not in (1, 2) or (stride == 2 and size is None):
        raise ValueError("%s: stride must be 1 or 2, got %r" % (who, stride))
    ok = dz.dim() == 4 and w.dim() in (2, 4) and w.size(0) == dz.size(1) and w.numel() == w.size(0) * w.size(1) * k * k and w.dtype == dz.dtype == torch.float32
    H, W = (dz.size(2), dz.size(3)) if ok else (0, 0)
    if ok and stride == 2:
        if y is not None and y.dim() == 4:
            H, W = y.size(2), y.size(3)
        elif in_hw is not None:
            H, W = int(in_hw[0]), int(in_hw[1])
        else:
            raise ValueError("%s: stride 2 needs the size of the conv's input map: pass y or in_hw=(H, W)" % who)
        ok = H >= 1 and W >= 1 and (dz.size(2), dz.size(3)) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1) and (in_hw is None or (H, W) == (int(in_hw[0]), int(in_hw[1])))
    if ok and y is not None:
        ok = y.dtype == torch.float32 and tuple(y.shape) == (dz.size(0), w.size(1), H, W)
    if not ok:
        raise ValueError("%s: expected float32 w [Cout,Cin%s], dz [B,Cout,%s] and y [B,Cin,H,W], got %s, %s and %s"
                         % (who, "" if size is None else ",%d,%d" % (k, k), "(H-1)//2+1,(W-1)//2+1" if stride == 2 else "H,W", tuple(w.shape), tuple(dz.shape),
                            None if y is None else tuple(y.shape)))
    return w.contiguous(), dz.contiguous(), None if y is None else y.contiguous(), H, W


def _dgrad(who, w, dz, size, row_scale, y, slope, stride=1, in_hw=None, thin=False):
    """The body of ``conv1x1_dgrad_async`` (``size`` None: rtod_conv1x1_dgrad, shape (B, Cout, Cin, pixels), no scale) and
    ``conv_dgrad_async`` (rtod_conv_dgrad, shape (B, Cout, Cin, H, W, size); ``stride`` 2: rtod_conv_dgrad_s2, H x W the conv's INPUT
    map): the tensor checks, the output, the launch.  ``thin``: rtod_conv_dgrad_thin (any Cin, stride 1)."""
    w, dz, y, H, W = _dgrad_operands(who, w, dz, size, y, stride, in_hw)
    B, cout, cin = dz.size(0), dz.size(1), w.size(1)
    shape = (B, cout, cin, H * W) if size is None else (B, cout, cin, H, W, int(size))
    dev = dz.device
    name = _DGRAD_ENTRIES.get((size is None, stride, bool(thin)))
    if name is None:
        raise ValueError("%s: the thin entry takes a size and stride 1" % who)
    dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dev)
    scale = () if size is None else (_scale_ptr(row_scale, cout, dev),)
    _ffi.enqueue(name, dev, w, *scale, dz, y, float(slope), *shape, dx)
    return dx


def conv1x1_dgrad_async(w, dz, y=None, slope=1.0):
    """Enqueue rtod_conv1x1_dgrad: ``w`` [Cout,Cin(,1,1)], ``dz`` [B,Cout,H,W] and, for a leaky layer, ``y`` [B,Cin,H,W] (the STORED
    output of the layer the conv reads) -> ``dx`` [B,Cin,H,W] = ``m(y) * W^T dz`` with ``m = 1`` where ``y > 0`` and ``slope``
    elsewhere.  Contiguous float32 device tensors, Cin a multiple of 32; nothing synchronises."""
    return _dgrad("conv1x1_dgrad", w, dz, None, None, y, slope)


def conv_dgrad_async(w, dz, size, row_scale=None, y=None, slope=1.0, stride=1, in_hw=None):
    """Enqueue rtod_conv_dgrad: ``w`` [Cout,Cin,size,size] (raw float32 masters), ``dz`` [B,Cout,H,W] and, for a leaky producer, ``y``
    [B,Cin,H,W] (the STORED output of the layer the conv reads) -> ``dx`` [B,Cin,H,W] = ``m(y) * conv_transpose(dz, v)`` of a ``size``
    x ``size`` (1 or 3), stride-1, same-padding conv with ``v = float32(float64(w) * row_scale[o])`` (``row_scale``: None, a float64
    device tensor [Cout] or the device address ``Darknet.conv_scale`` returns).  Contiguous float32 device tensors, Cin a multiple
    of 32; one fmaf chain per tap, the tap sums added in ascending order: an order the shape fixes; nothing synchronises.
    ``stride`` 2 (rtod_conv_dgrad_s2): a 3x3 / stride-2 / pad-1 conv, ``dz`` [B,Cout,Ho,Wo] on its output map and ``dx`` on its
    INPUT map, whose size comes from ``y``, else from ``in_hw = (H, W)``: ``Ho`` alone does not tell ``2 Ho`` from ``2 Ho - 1``.
    A ``Cin`` that is no multiple of 32 goes to the entry of ``conv_dgrad_thin_async`` (stride 1), and only such a one."""
    thin = isinstance(w, torch.Tensor) and w.dim() in (2, 4) and w.size(1) % 32 != 0
    return _dgrad("conv_dgrad_thin" if thin else "conv_dgrad", w, dz, int(size), row_scale, y, slope, stride, None if thin else in_hw, thin)


def conv_dgrad_thin_async(w, dz, size, row_scale=None, y=None, slope=1.0, stride=1):
    """Enqueue rtod_conv_dgrad_thin: ``conv_dgrad_async`` for a 1x1 or 3x3 / stride-1 conv of ANY ``Cin`` (YOLOv3-tiny's layer 2
    reads 16 channels): the same chain per tap, tap order and mask, rows past ``Cin`` staged as zeros and never stored."""
    return _dgrad("conv_dgrad_thin", w, dz, int(size), row_scale, y, slope, stride, None, thin=True)


GRAD_PRECISIONS = ("fp32", "f16s3")      # DarknetTrainer(grad_precision=...): the exact data gradients, or the split-f16 ones where the walk sends the conv there
# ... which is the 3x3 convs the entry takes.  The 1x1 convs stay on the exact entry: measured (tools/exp_grad_split.py, profiles/experiments/grad_split_cost.log;
# 416x416 batch 8) YOLOv3's 37 take 2033.6 us exact and 1786.5 us through the split entry, YOLOv3-tiny's 4 take 95.3 us exact and 129.6 us split (four helper
# launches per call around a small GEMM), and YOLOv3's whole step is the same within the rounds' spread either way (34151.8 us with them, 34207.7 us without)
GRAD_SPLIT_SIZES = (3,)


def conv_dgrad_split_tiles(batch, cout, cin, height, width, size):
    """The legal tile ids of rtod_conv_dgrad_split for that shape, the default first (rtod_conv_dgrad_split_tiles; no device)."""
    lib = _ffi.lib()
    shape = (int(batch), int(cout), int(cin), int(height), int(width), int(size))
    n = lib.rtod_conv_dgrad_split_tiles(*shape, None, 0)
    if n < 0:
        _ffi.check(n)
    ids = (C.c_int * max(n, 1))()
    n = lib.rtod_conv_dgrad_split_tiles(*shape, ids, n)
    if n < 0:
        _ffi.check(n)
    return [ids[i] for i in range(n)]


def conv_dgrad_split_takes(cin, size, stride=1):
    """Does rtod_conv_dgrad_split take a conv of that shape?  Stride 1, size 1 or 3, ``Cin`` a positive multiple of 32."""
    return stride == 1 and size in (1, 3) and cin >= 32 and cin % 32 == 0


def conv_dgrad_split_async(w, dz, size, row_scale=None, y=None, slope=1.0, tile=None, phases=None):
    """Enqueue rtod_conv_dgrad_split: the operands and the result of ``conv_dgrad_async`` (stride 1, ``Cin`` a multiple of 32), summed
    on the forward's split-f16 MFMA tiles: ``dz`` scaled per image by a power of two and split into f16 hi / lo planes, the weights
    packed transposed, flipped and pre-scaled per row from the masters at every call, hi*hi + hi*lo + lo*hi in fp32 accumulators, then
    exact inverse scales and one multiplication by the mask.  ``tile``: one of ``conv_dgrad_split_tiles`` (None: the default; every
    legal tile gives the same bits).  The workspace is cached per shape; nothing synchronises.  ``phases`` (measurement only,
    rtod_conv_dgrad_split_phases): a sum of 1, 2, 4, 8, 16 naming the kernel groups to enqueue on the workspace a full call has filled."""
    w, dz, y, H, W = _dgrad_operands("conv_dgrad_split", w, dz, int(size), y)
    B, cout, cin = dz.size(0), dz.size(1), w.size(1)
    shape = (B, cout, cin, H, W, int(size))
    dev = dz.device
    dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_conv_dgrad_split" if phases is None else "rtod_conv_dgrad_split_phases", dev, w, _scale_ptr(row_scale, cout, dev), dz, y, float(slope),
                 *shape, -1 if tile is None else int(tile), dx, *_ffi.workspace("rtod_conv_dgrad_split", dev, *shape), after=() if phases is None else (int(phases),))
    return dx


WGRAD_PRECISIONS = ("fp32", "f16s3")     # DarknetTrainer(wgrad_precision=...): the exact weight gradients, or the split-f16 ones where the walk sends the conv there
# ... which is the stride-1 3x3 BatchNorm convs the entry takes.  Settled by tools/exp_wgrad_split.py (profiles/experiments/wgrad_split_cost.log): a size stays only
# if its summed split time is below its summed exact time on YOLOv3 416x416 batch 8.  Its 32 3x3 layers take 9136.2 us exact and 5087.6 us through the split entry;
# its 34 1x1 layers take 2739.7 us exact and 2790.5 us split (on YOLOv3-tiny 47.3 against 71.8 us): two planes written and read back around one tap's worth of
# MFMAs, so the 1x1 convs stay on the exact entry.  The ENTRY takes them and the tests cover them
WGRAD_SPLIT_SIZES = (3,)


def conv_wgrad_split_takes(cin, size, stride=1):
    """Does rtod_conv_wgrad_split take a conv of that shape?  Stride 1, size 1 or 3, ``Cin`` a positive multiple of 32."""
    return stride == 1 and size in (1, 3) and cin >= 32 and cin % 32 == 0


def conv_wgrad_split_schedule(batch, cout, cin, height, width, size):
    """``(tiles, slices, slice_len, k_padded)`` of rtod_conv_wgrad_split for that shape (rtod_conv_wgrad_split_schedule; no device)."""
    t, s, n, k = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    _ffi.check(_ffi.lib().rtod_conv_wgrad_split_schedule(int(batch), int(cout), int(cin), int(height), int(width), int(size), C.byref(t), C.byref(s), C.byref(n), C.byref(k)))
    return t.value, s.value, n.value, k.value


def conv_wgrad_split_async(dz, x, size, row_scale=None, phases=None):
    """Enqueue rtod_conv_wgrad_split: the operands of ``conv_wgrad_async`` (stride 1, no bias gradient, ``Cin`` a multiple of 32) ->
    ``dW [Cout,Cin,size,size]`` summed as three f16 MFMA products: ``dz`` and ``x`` scaled by ONE power of two per tensor and split
    into f16 hi / lo planes on a common padded k grid, hi*hi + hi*lo + lo*hi in fp32 accumulators, K slices added in ascending
    order, then ``2^-(e_z + e_x) * row_scale[o]`` once in double.  The workspace is cached per shape; nothing synchronises.
    ``phases`` (measurement only, rtod_conv_wgrad_split_phases): a sum of 1, 2, 4, 8 naming the kernel groups to enqueue on the
    workspace a full call has filled."""
    who = "conv_wgrad_split"
    _need_cuda(dz, who)
    _need_cuda(x, who)
    ok = dz.dim() == 4 and x.dim() == 4 and dz.size(0) == x.size(0) and dz.dtype == torch.float32 and x.dtype == torch.float32 and tuple(dz.shape[2:]) == tuple(x.shape[2:])
    if not ok:
        raise ValueError("%s: expected float32 dz [B,Cout,H,W] and x [B,Cin,H,W], got %s and %s" % (who, tuple(dz.shape), tuple(x.shape)))
    dz, x = dz.contiguous(), x.contiguous()
    B, cout, cin, H, W = dz.size(0), dz.size(1), x.size(1), x.size(2), x.size(3)
    shape = (B, cout, cin, H, W, int(size))
    dev = dz.device
    scale = _scale_ptr(row_scale, cout, dev)
    ws = _ffi.workspace("rtod_conv_wgrad_split", dev, *shape)         # a refused shape raises here: nothing is launched
    dw = torch.empty((cout, cin, int(size), int(size)), dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_conv_wgrad_split" if phases is None else "rtod_conv_wgrad_split_phases", dev, dz, x, *shape, scale, dw, *ws,
                 after=() if phases is None else (int(phases),))
    return dw


def maxpool_grad_async(dz, x, slope=1.0, size=2, stride=2):
    """Enqueue rtod_maxpool_grad: ``dz`` on the pool's output map ([B,C,H//2,W//2] for ``stride`` 2, [B,C,H,W] for the clamped
    ``stride`` 1 pool) and ``x`` [B,C,H,W], the pool's stored input -> ``dx`` [B,C,H,W]: every window's gradient goes to its first
    maximum (the forward's and torch's rule), contributions added in ascending window order, then times ``m(x)`` (1 where ``x > 0``,
    else ``slope``: the leaky mask of the conv that produced ``x``).  Gather form, no atomics; contiguous float32 device tensors;
    nothing synchronises."""
    for t in (dz, x):
        _need_cuda(t, "maxpool_grad")
    ok = dz.dim() == 4 and x.dim() == 4 and dz.dtype == x.dtype == torch.float32 and tuple(dz.shape[:2]) == tuple(x.shape[:2])
    if ok and stride in (1, 2):
        ok = tuple(dz.shape[2:]) == (tuple(x.shape[2:]) if stride == 1 else (x.size(2) // 2, x.size(3) // 2))
    if not ok:
        raise ValueError("maxpool_grad: expected float32 dz on the pool's output map and x [B,C,H,W], got %s and %s (stride %r)" % (tuple(dz.shape), tuple(x.shape), stride))
    dz, x = dz.contiguous(), x.contiguous()
    B, ch, H, W = x.shape
    dev = x.device
    dx = torch.empty((B, ch, H, W), dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_maxpool_grad", dev, dz if dz.numel() else None, x, float(slope), B, ch, H, W, int(size), int(stride), dx)
    return dx


def bn_grad_parts(batch, channels, pixels):
    """``(parts, part_len)`` of rtod_bn_grad for that shape (rtod_bn_grad_parts): a channel's ``batch * pixels`` values are summed as
    ``parts`` contiguous ranges of ``part_len``, a rule of the shape alone."""
    p, n = C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().rtod_bn_grad_parts(int(batch), int(channels), int(pixels), C.byref(p), C.byref(n)))
    return p.value, n.value


def _stat_ptr(who, t, channels, dev):
    """``mean`` / ``var`` of ``bn_grad_async`` as a pointer argument: a contiguous float64 device tensor [C] (checked), or an integer
    device address."""
    if isinstance(t, torch.Tensor):
        if t.device != dev or t.dtype != torch.float64 or t.numel() != channels or not t.is_contiguous():
            raise ValueError("%s: mean and var must be contiguous float64 tensors [%d] on %s" % (who, channels, dev))
        return t
    return int(t)


def bn_grad_async(du, z, mean, var, gamma):
    """Enqueue rtod_bn_grad, the backward of batch-statistics BatchNorm: ``du`` [B,C,H,W] (the gradient with respect to the BatchNorm
    output, the leaky mask already applied), ``z`` [B,C,H,W] (the raw conv output the forward normalised), ``mean`` / ``var`` (float64
    device tensors [C] or integer device addresses: the doubles the forward normalised with) and ``gamma`` (float32 [C]) ->
    ``(dz [B,C,H,W], dgamma [C], dbeta [C])``.  Double sums over a partition the shape alone fixes (``bn_grad_parts``), two launches,
    no atomics: bit-identical from call to call.  Contiguous float32 device tensors; the workspace is cached per shape; nothing
    synchronises."""
    for t in (du, z, gamma):
        _need_cuda(t, "bn_grad")
    if du.dim() != 4 or tuple(du.shape) != tuple(z.shape) or du.dtype != torch.float32 or z.dtype != torch.float32 or gamma.dtype != torch.float32 \
            or gamma.numel() != du.size(1):
        raise ValueError("bn_grad: expected float32 du and z [B,C,H,W] and gamma [C], got %s, %s and %s" % (tuple(du.shape), tuple(z.shape), tuple(gamma.shape)))
    aligned = lambda t: t.contiguous() if t.contiguous().data_ptr() % 16 == 0 else t.contiguous().clone()
    du, z, gamma = aligned(du), aligned(z), gamma.contiguous()
    B, ch, pixels = du.size(0), du.size(1), du.size(2) * du.size(3)
    dev = du.device
    dz = torch.empty_like(du)
    dgamma = torch.empty(ch, dtype=torch.float32, device=dev)
    dbeta = torch.empty(ch, dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_bn_grad", dev, du, z, _stat_ptr("bn_grad", mean, ch, dev), _stat_ptr("bn_grad", var, ch, dev), gamma, B, ch, pixels,
                 dz, dgamma, dbeta, *_ffi.workspace("rtod_bn_grad", dev, B, ch, pixels))
    return dz, dgamma, dbeta


def grad_join_async(contributions, y=None, slope=1.0):
    """Enqueue rtod_grad_join: ``m(y) * (((c0 + c1) + c2) + c3)`` over equally shaped contiguous float32 device tensors, float32
    adds from left to right, then one multiplication by ``slope`` where ``not (y > 0)`` (``y`` None or ``slope`` 1: no mask) — the
    bits of ``(c0 + c1 + ...) * full_like(y, slope).masked_fill_(y > 0, 1)`` in one launch.  More than four contributions go
    through several launches in the same order, the mask in the last.  A new tensor; nothing synchronises."""
    cs = list(contributions)
    if not cs:
        raise ValueError("grad_join: no contribution")
    for t in cs + ([y] if y is not None else []):
        _need_cuda(t, "grad_join")
        if t.dtype != torch.float32 or tuple(t.shape) != tuple(cs[0].shape):
            raise ValueError("grad_join: expected equally shaped float32 tensors, got %s and %s" % (tuple(cs[0].shape), tuple(t.shape)))
    cs = [c.contiguous() for c in cs]
    y = None if y is None else y.contiguous()
    dev = cs[0].device
    while True:
        now, cs = cs[:4], cs[4:]
        last = not cs
        out = torch.empty_like(now[0])
        ptrs = (C.c_void_p * 4)(*[c.data_ptr() for c in now])
        _ffi.enqueue("rtod_grad_join", dev, ptrs, len(now), y if last else None, float(slope) if last else 1.0, out.numel(), out)
        if last:
            return out
        cs = [out] + cs


def upsample2x_grad_async(dz, y=None, slope=1.0, mode="bilinear"):
    """Enqueue rtod_upsample2x_grad: ``dz`` [B,C,2H,2W] -> ``dx`` [B,C,H,W], the backward of the 2x upsample (``mode`` "bilinear":
    align_corners=False, or "nearest") in gather form without atomics, times ``m(y)`` for a leaky producer's stored output ``y``
    [B,C,H,W].  Contiguous float32 device tensors; nothing synchronises."""
    for t in (dz,) + ((y,) if y is not None else ()):
        _need_cuda(t, "upsample2x_grad")
    if mode not in ("bilinear", "nearest"):
        raise ValueError("upsample2x_grad: mode must be 'bilinear' or 'nearest', got %r" % (mode,))
    ok = dz.dim() == 4 and dz.dtype == torch.float32 and dz.size(2) % 2 == 0 and dz.size(3) % 2 == 0
    if ok and y is not None:
        ok = y.dtype == torch.float32 and tuple(y.shape) == (dz.size(0), dz.size(1), dz.size(2) // 2, dz.size(3) // 2)
    if not ok:
        raise ValueError("upsample2x_grad: expected float32 dz [B,C,2H,2W] and y [B,C,H,W], got %s and %s" % (tuple(dz.shape), None if y is None else tuple(y.shape)))
    dz = dz.contiguous()
    y = None if y is None else y.contiguous()
    B, ch, H, W = dz.size(0), dz.size(1), dz.size(2) // 2, dz.size(3) // 2
    dev = dz.device
    dx = torch.empty((B, ch, H, W), dtype=torch.float32, device=dev)
    _ffi.enqueue("rtod_upsample2x_grad", dev, dz, y, float(slope), 1 if mode == "nearest" else 0, B, ch, H, W, dx)
    return dx


def model_heads(model, height=None, width=None):
    """``[(grid_h, grid_w, stride, anchors)]`` of a Darknet's [yolo] layers in cfg order, and its number of classes."""
    h = int(model.net_info["height"]) if height is None else int(height)
    w = (int(model.input_width) if getattr(model, "input_width", None) is not None else h) if width is None else int(width)
    heads, classes = [], None
    for L in build_ir(model.blocks, h, w).layers:
        if L.type != "yolo":
            continue
        if L.decode_v5:
            raise ValueError("DarknetTrainer: a [yolo] layer with decode=v5 has no TRAIN=True decode; the reference's loss is not defined for it")
        heads.append((L.hout, L.wout, h // L.hout, [tuple(a) for a in L.anchors]))
        classes = L.classes
    if not heads:
        raise ValueError("DarknetTrainer: the cfg has no [yolo] layer")
    return heads, classes


def batch_mode(model):
    """Batch mode: the model normalises with the statistics of the batch (``.train()``, ``bn_running_stats_in_train`` off) and its
    plan keeps the BatchNorm inputs (option ``keep_bn_inputs``), so the walk goes through ``bn_grad_async`` and gamma and beta are
    trained.  Otherwise BatchNorm is frozen (an eval model)."""
    return bool(getattr(model, "training", False) and not getattr(model, "bn_running_stats_in_train", False)
                and int(getattr(model, "options", {}).get("keep_bn_inputs", 0)))


def conv_kind(model, layer):
    """The kind of a trained conv, a key of ``darknet.CONV_KINDS``, decided here and nowhere else: "head" (no BatchNorm: weight and
    bias), "bn" (BatchNorm on batch statistics in batch mode: weight, gamma, beta) or "folded" (BatchNorm frozen: weight alone)."""
    return "head" if model._conv_bn(layer)[1] is None else "bn" if batch_mode(model) else "folded"


# A conv's masters (``DarknetTrainer._head_masters[layer]``) and its gradients (``HeadOptimizer.step``) are lists with one slot per
# parameter name, cut after the last one the kind has: [weight, bias or None(, gamma, beta)].  ``HeadOptimizer.state`` names them in
# torch's words; the moments of "weight" carry no suffix.
_SLOT = {"weight": 0, "bias": 1, "gamma": 2, "beta": 3}
_STATE_KEY = {"weight": "weight", "bias": "bias", "gamma": "bn_weight", "beta": "bn_bias"}


def _slots(kind, named):
    """``{parameter name: tensor}`` of a conv of ``kind`` as its list of slots."""
    out = [None] * (1 + max(_SLOT[name] for name in CONV_KINDS[kind].params + ("bias",)))
    for name in CONV_KINDS[kind].params:
        out[_SLOT[name]] = named[name]
    return out


def _moment_keys(name):
    return tuple(m + ("" if name == "weight" else "_" + _STATE_KEY[name]) for m in ("exp_avg", "exp_avg_sq"))


class HeadOptimizer:
    """Adam (the reference's ``optim.Adam(self.darknet.parameters(), lr=1e-2)``, train.py:57: no weight decay, no amsgrad) or plain
    SGD on the detection-head convs, run by ``Darknet.step_conv``: one kernel per conv that steps the float32 masters and re-packs
    the conv's block of the plan's weight image in place; nothing synchronises.

    ``state``: ``{conv_layer: {"step": t, "weight", "bias", "exp_avg", "exp_avg_sq", "exp_avg_bias", "exp_avg_sq_bias"}}`` — the
    masters (the very tensors of ``DarknetTrainer._head_masters``, so ``head_step`` and this path can be mixed), torch's moment
    names and the number of steps taken; SGD keeps no moments.  ``lr`` may be changed between steps.  A conv whose BatchNorm runs on
    batch statistics (the trainer's batch mode, ``Darknet.step_conv_bn``) also keeps ``bn_weight`` and ``bn_bias`` (the gamma and beta
    masters) and, for Adam, ``exp_avg_bn_weight``, ``exp_avg_sq_bn_weight``, ``exp_avg_bn_bias``, ``exp_avg_sq_bn_bias``;
    ``state_dict`` / ``load_state_dict`` carry them like the rest."""

    KINDS = {"sgd": 0, "adam": 1}

    def __init__(self, kind="adam", lr=1e-2, betas=(0.9, 0.999), eps=1e-8):
        if kind not in self.KINDS:
            raise ValueError("HeadOptimizer: kind must be 'adam' or 'sgd', got %r" % (kind,))
        self.kind, self.lr, self.betas, self.eps = kind, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.state = {}
        self._trainer = None               # weak reference to the DarknetTrainer this optimiser is the ``optimizer`` of

    def _entry(self, kind, layer, masters):
        """The state of a conv of ``kind``: its masters adopted (new weight or bias masters start the moments afresh, the step count
        stays), for Adam the moments of every parameter the kind has."""
        st = self.state.get(layer)
        if st is None or st["weight"] is not masters[0] or st.get("bias") is not masters[1]:
            st = self.state[layer] = {"step": 0 if st is None else st["step"]}
        names = CONV_KINDS[kind].params
        for name in names:
            st[_STATE_KEY[name]] = masters[_SLOT[name]]
        if self.kind == "adam":
            for name in names:
                for key in _moment_keys(name):
                    if key not in st:
                        st[key] = torch.zeros_like(st[_STATE_KEY[name]])
        return st

    def step(self, model, masters, grads):
        """One step of every conv in ``grads`` on ``masters``: ``{conv_layer: (dW, db)}`` and ``{conv_layer: [weight, bias]}`` for a
        head conv (``Darknet.step_conv``), ``(dW, None)`` and ``[weight, None]`` for a block conv (``Darknet.step_conv_folded``),
        ``(dW, None, dgamma, dbeta)`` and ``[weight, None, gamma, beta]`` for a conv whose BatchNorm runs on batch statistics
        (``Darknet.step_conv_bn``)."""
        for layer, grad in grads.items():
            kind = conv_kind(model, layer)
            K = CONV_KINDS[kind]
            st = self._entry(kind, layer, masters[layer])
            st["step"] += 1
            opt = _ffi.OptStep(self.KINDS[self.kind], self.lr, self.betas[0], self.betas[1], self.eps, st["step"])
            operands = [grad[_SLOT[name[2:]]] if name.startswith("d.") else st[_STATE_KEY[name]] for name in K.order]
            moments = tuple(st[key] for name in K.params for key in _moment_keys(name)) if self.kind == "adam" else None
            getattr(model, K.step)(layer, opt, *operands, moments)

    def state_dict(self):
        """``{conv_layer: {"step": int, name: tensor}}`` of the masters and moments (the tensors themselves, as torch's does)."""
        return {layer: dict(st) for layer, st in self.state.items()}

    def load_state_dict(self, state):
        """Take copies of a ``state_dict()``'s tensors.  As a trainer's ``optimizer`` it also makes the masters that trainer's and
        hands them to its model (``Darknet.update_conv`` per conv: synchronises), so a second trainer continues where the first
        one's state was taken."""
        self.state = {int(layer): {k: (v.detach().clone() if isinstance(v, torch.Tensor) else int(v)) for k, v in st.items()} for layer, st in state.items()}
        trainer = self._trainer() if self._trainer is not None else None
        if trainer is not None:
            trainer._head_masters = {}
            for layer, st in self.state.items():
                kind = conv_kind(trainer.darknet, layer)
                named = {name: st[_STATE_KEY[name]] for name in CONV_KINDS[kind].params}
                trainer._head_masters[layer] = _slots(kind, named)
                getattr(trainer.darknet, CONV_KINDS[kind].update)(layer, *named.values())


class DarknetTrainer:
    """The loss side of the reference's trainer around a built ``Darknet`` (no optimiser, no epochs, no data loaders).

    Attributes (the reference's): darknet, resolution, num_classes, criterion, TINY, history, optimizer (a ``HeadOptimizer``: the
    heads alone are trained).  New: ``heads`` (from the cfg),
    ``min_box_size`` (the literal 24 of target_layer), ``status`` (device int32 [1]: bit 0 = a box's cell lay outside a grid and
    was skipped; OR-ed by every call, read it when you synchronise anyway), ``last_components`` (device float64 [6] of the
    last loss: total, xy, wh, obj, noobj, cls)."""

    def __init__(self, model, resolution=None, num_classes=None, trainable="heads", grad_precision="fp32", wgrad_precision="fp32"):
        if trainable not in ("heads", "blocks", "neck", "backbone", "full"):
            raise ValueError("DarknetTrainer: trainable must be 'heads', 'blocks', 'neck', 'backbone' or 'full', got %r" % (trainable,))
        if grad_precision not in GRAD_PRECISIONS:
            raise ValueError("DarknetTrainer: grad_precision must be 'fp32' or 'f16s3', got %r" % (grad_precision,))
        if wgrad_precision not in WGRAD_PRECISIONS:
            raise ValueError("DarknetTrainer: wgrad_precision must be 'fp32' or 'f16s3', got %r" % (wgrad_precision,))
        self.wgrad_precision = wgrad_precision  # "f16s3": _walk sends dW of every stride-1 BatchNorm conv with a size in WGRAD_SPLIT_SIZES and Cin % 32 == 0 through
                                           # conv_wgrad_split_async; head convs, stride 2 and thin convs stay exact.  Independent of grad_precision
        self.grad_precision = grad_precision   # "f16s3": _walk sends the data gradient of every stride-1 3x3 conv with Cin % 32 == 0 through
                                           # conv_dgrad_split_async; 1x1 convs (GRAD_SPLIT_SIZES), stride 2, thin convs, weight gradients, BatchNorm and joins stay exact
        self.trainable = trainable         # "blocks": feed_forward_through_model also trains the BatchNorm conv in front of each head conv;
                                           # "neck": every BatchNorm conv behind the backbone (Darknet.neck_layers);
                                           # "backbone": every conv the plan can train (Darknet.trainable_layers: all but layer 0 on YOLOv3)
                                           # "full": ... through thin convs and max-pools too (Darknet.full_layers: all 11 BatchNorm convs of YOLOv3-tiny)
        self.darknet = model
        if resolution is not None:
            assert isinstance(resolution, int) and resolution % 32 == 0
            model.net_info["height"] = resolution
        self.resolution = int(model.net_info["height"])
        self.heads, classes = model_heads(model)
        self.num_classes = int(classes if num_classes is None else num_classes)
        if self.num_classes != classes:
            raise ValueError("DarknetTrainer: num_classes=%d but the cfg's [yolo] layers have %d" % (self.num_classes, classes))
        self.TINY = len(self.heads) == 2
        self.min_box_size = 24
        self.criterion = self.darknet_loss
        self.history = dict()
        self.status = None
        self.last_components = None
        self._head_masters = None          # head_step / optimizer: {conv_layer: [weight, bias]} float32 device masters of the head convs
        self._net_input = None             # the prepared input of the last _forward_train (what layer 0 read)
        self._graph_cache = None           # gradients: (scope, plan and weight version, the graph of that scope with its scales)
        self.optimizer = HeadOptimizer()
        self._require_bn_option("DarknetTrainer", trainable)

    # ------------------------------------------------------------------ BatchNorm on batch statistics: the one place that decides the mode
    def _batch_stats(self):
        """The model normalises with the statistics of the batch (``.train()``, ``bn_running_stats_in_train`` off)."""
        m = self.darknet
        return bool(getattr(m, "training", False) and not getattr(m, "bn_running_stats_in_train", False))

    def _batch_mode(self):
        return batch_mode(self.darknet)

    def _require_bn_option(self, who, scope):
        if scope in self.SCOPES and self._batch_stats() and not self._batch_mode():
            raise RuntimeError("%s: the model is in .train() (BatchNorm on batch statistics) and scope %r trains BatchNorm convs: set "
                               "model.options['keep_bn_inputs'] = 1 before the first forward (the BatchNorm backward reads the raw conv outputs), "
                               "or call .eval() to train with BatchNorm frozen" % (who, scope))

    @property
    def optimizer(self):
        return self._optimizer

    @optimizer.setter
    def optimizer(self, opt):
        opt._trainer = weakref.ref(self)
        self._optimizer = opt

    # ------------------------------------------------------------------ host mirrors (small and exact)
    @staticmethod
    def anchor_fit(box, anchors):
        """Index of the best fitting anchor (train.py:196-209): first maximum of the IoU of the box's (w, h) with a square of
        the anchor's width — bbox_iou_wh reads the anchor's width twice — in Python floats."""
        w1, h1 = float(np.float32(box[2])), float(np.float32(box[3]))
        best, best_iou = 0, None
        for i, anchor in enumerate(anchors):
            w2 = h2 = float(anchor[0])
            inter = min(w1, w2) * min(h1, h2)
            iou = inter / (w1 * h1 + w2 * h2 - inter)
            if best_iou is None or iou > best_iou:
                best, best_iou = i, iou
        return best

    def target_layer(self, bboxes, scale, anchors):
        """Target and mask of one square head (train.py:167-193) on the host: float32 ``[scale*scale*A, 5+C]`` and ``[...]``."""
        A = len(anchors)
        output = torch.zeros((scale * scale * A, 5 + self.num_classes))
        mask = torch.zeros(output.shape[:-1])
        stride = self.resolution // scale
        boxes = np.asarray(torch.as_tensor(bboxes, dtype=torch.float32).cpu().numpy(), np.float32).reshape(-1, 5 + self.num_classes)
        for box in boxes:
            if box[5] != 1 or box[2] < np.float32(self.min_box_size) or box[3] < np.float32(self.min_box_size):
                continue
            fit = self.anchor_fit(box, anchors)
            x, y = float(box[0]) / stride, float(box[1]) / stride
            if not (0.0 <= x < scale and 0.0 <= y < scale):
                continue                                              # outside the grid: skipped (the reference wraps or raises)
            gx, gy = int(x), int(y)
            loc = (gy * scale + gx) * A + fit
            row = box.copy()
            row[0], row[1] = np.float32(y - gy), np.float32(x - gx)      # the reference's swapped centre slots
            with np.errstate(divide="ignore"):
                row[2] = np.float32(math.log(float(box[2] / np.float32(anchors[fit][0]) + np.float32(1e-16))))
                row[3] = np.float32(math.log(float(box[3] / np.float32(anchors[fit][1]) + np.float32(1e-16))))
            output[loc] = torch.from_numpy(row)
            mask[loc] = 1
        return output, mask

    # ------------------------------------------------------------------ device paths
    def _status(self, dev):
        if self.status is None or self.status.device != dev:
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        return self.status

    def _device(self):
        if not torch.cuda.is_available():
            raise RuntimeError("DarknetTrainer: this build has no CPU path")
        return torch.device("cuda", torch.cuda.current_device())

    def target_creator(self, bndbox):
        """``(target float32 [B,N,5+C], mask bool [B,N])`` as device tensors (train.py:129-149), written by the kernels."""
        dev = next((t.device for t in bndbox if isinstance(t, torch.Tensor) and t.is_cuda), None) or self._device()
        n = sum(gh * gw * len(a) for gh, gw, _, a in self.heads)
        pred = torch.zeros((len(bndbox), n, 5 + self.num_classes), dtype=torch.float32, device=dev)
        out = yolo_loss_async(pred, bndbox, self.heads, self.num_classes, self.min_box_size, dense=True, status=self._status(dev))
        return out["target"], out["mask"].bool()

    def darknet_loss(self, pred, target, obj_mask):
        """The loss of dense tensors (train.py:211-230) as a 0-dim float32 device tensor; ``last_components`` holds the doubles."""
        _need_cuda(pred, "darknet_loss")
        _need_cuda(target, "darknet_loss")
        if not isinstance(obj_mask, torch.Tensor) or not obj_mask.is_cuda:
            raise RuntimeError("darknet_loss: expected a CUDA (ROCm) mask; this build has no CPU path")
        if pred.shape != target.shape or pred.dim() < 2 or tuple(obj_mask.shape) != tuple(pred.shape[:-1]):
            raise ValueError("darknet_loss: pred %s, target %s and obj_mask %s do not fit" % (tuple(pred.shape), tuple(target.shape), tuple(obj_mask.shape)))
        pred, target = pred.contiguous(), target.contiguous()
        mask = (obj_mask if obj_mask.dtype == torch.uint8 else obj_mask.bool().to(torch.uint8)).contiguous()
        attrs = pred.size(-1)
        rows = pred.numel() // attrs
        dev = pred.device
        comp = torch.empty(6, dtype=torch.float64, device=dev)
        _ffi.enqueue("rtod_darknet_loss_dense", dev, pred, target, mask, rows, attrs, comp, *_workspace(dev, 1, rows))
        self.last_components = comp
        return comp[0].float()

    def loss_from_boxes(self, pred, bndbox):
        """``(loss, components)`` of a TRAIN=True prediction tensor against per-image box lists, without a dense target: loss a
        0-dim float32 device tensor, components the device float64 [6] (total, xy, wh, obj, noobj, cls).  Nothing synchronises."""
        out = yolo_loss_async(pred, bndbox, self.heads, self.num_classes, self.min_box_size, status=self._status(pred.device))
        self.last_components = out["components"]
        return out["components"][0].float(), out["components"]

    def forward_loss(self, frames_or_x, bndbox):
        """Forward under ``train_mode()`` (float32 ``[B,3,H,W]`` inputs, or uint8 ``[B,H,W,3]`` RGB frames letterboxed on the
        device), then ``loss_from_boxes``; returns the loss."""
        return self.loss_from_boxes(self._forward_train(frames_or_x), bndbox)[0]

    # ------------------------------------------------------------------ gradients of the detection-head convs
    def _forward_train(self, frames_or_x):
        x = torch.as_tensor(frames_or_x)
        if x.dtype == torch.uint8:
            h = int(self.darknet.net_info["height"])
            w = int(self.darknet.input_width) if getattr(self.darknet, "input_width", None) is not None else h
            x = prep_frames(x, (w, h), mode="RGB")
        elif not x.is_cuda:
            x = x.cuda()
        self._net_input = x
        with torch.no_grad(), self.darknet.train_mode():
            return self.darknet(x)

    def head_gradients(self, frames_or_x, bndbox):
        """``(loss, {conv_layer: (dW [Cout,Cin,1,1], db [Cout])})``: what ``loss.backward()`` of the reference leaves on the
        detection-head convs.  Forward under ``train_mode()`` (inputs as ``forward_loss``), rtod_yolo_loss_grad, then per head
        ``read_layer`` of the conv's input and rtod_conv1x1_wgrad; all on the current stream, nothing synchronises.  The model's
        ``options`` must hold ``keep_head_inputs`` (the head inputs are otherwise overwritten before the forward ends)."""
        loss, grads, _ = self._head_pass(frames_or_x, bndbox)
        return loss, grads

    def _head_pass(self, frames_or_x, bndbox):
        """The body of ``head_gradients``, which ``gradients`` goes on from: ``(loss, {conv_layer: (dW, db)}, {conv_layer: (dz,
        x)})`` with dz the gradient of the head's raw map and x the dense copy of the head conv's input."""
        model = self.darknet
        if not int(getattr(model, "options", {}).get("keep_head_inputs", 0)):
            raise RuntimeError("DarknetTrainer.head_gradients: set model.options['keep_head_inputs'] = 1 before the first forward; "
                               "without it the activations that feed the head convs do not survive the forward")
        pred = self._forward_train(frames_or_x)                        # (leaves the prepared network input in _net_input: layer 0's dW reads it)
        out = yolo_loss_grad_async(pred, bndbox, self.heads, self.num_classes, self.min_box_size, status=self._status(pred.device))
        self.last_components = out["components"]
        layers = model.head_layers()
        if len(layers) != len(self.heads):
            raise RuntimeError("DarknetTrainer.head_gradients: %d [yolo] layers but %d of them follow a convolution" % (len(self.heads), len(layers)))
        grads, operands = {}, {}
        for (conv_layer, input_layer), dz in zip(layers, out["grad_raw"]):
            if input_layer < 0:
                raise RuntimeError("DarknetTrainer.head_gradients: head conv %d reads the network input" % conv_layer)
            x = model.read_layer(input_layer, pred.size(0))
            grads[conv_layer] = conv1x1_wgrad_async(dz, x)
            operands[conv_layer] = (dz, x)
        return out["components"][0].float(), grads, operands

    def head_step(self, frames_or_x, bndbox, lr):
        """One plain SGD step on the detection-head convs, ``w -= lr * dW``, ``b -= lr * db``, on float32 device masters the
        trainer keeps for them (taken from the model's parameters at the first call), followed by ``Darknet.update_conv``, which
        re-packs those convs alone.  SYNCHRONISES the device (the updated weights pass through the host).  Returns the loss
        from before the step (0-dim float32 device tensor)."""
        loss, grads = self.head_gradients(frames_or_x, bndbox)
        model = self.darknet
        masters = self._masters(grads, loss.device)
        for layer, (dw, db) in grads.items():
            w, b = masters[layer]
            w.sub_(dw * float(lr))
            b.sub_(db * float(lr))
            model.update_conv(layer, w, b)
        return loss

    def _masters(self, layers, dev):
        """The float32 device masters ``[weight, bias]`` of the trained convs (bias None for a block conv: it has BatchNorm), taken
        from the model's parameters the first time each is needed.  In batch mode a BatchNorm conv's entry is ``[weight, None, gamma,
        beta]``."""
        if self._head_masters is None:
            self._head_masters = {}
        kinds = {layer: conv_kind(self.darknet, layer) for layer in layers}
        missing = [layer for layer, kind in kinds.items() if layer not in self._head_masters or (kind == "bn" and len(self._head_masters[layer]) < 4)]
        if missing:
            self.darknet.sync_stepped_parameters()
            for layer in missing:
                K = CONV_KINDS[kinds[layer]]
                kept = self._head_masters.get(layer, ())                  # (a conv that was trained with BatchNorm frozen keeps its weight master)
                named = {name: kept[_SLOT[name]] if _SLOT[name] < len(kept) else p.detach().to(dev, torch.float32).clone()
                         for name, p in zip(K.params, self.darknet._params(kinds[layer], layer))}
                self._head_masters[layer] = _slots(kinds[layer], named)
        return self._head_masters

    # ------------------------------------------------------------------ gradients behind the heads: one entry, three scopes
    # scope -> (its named entry; the options that keep its activations: any one of them, beside keep_head_inputs; what is lost without them)
    SCOPES = {"blocks": ("block_gradients", ("keep_block_inputs",), "the activations that feed the head convs and the block convs do not survive the forward"),
              "neck": ("neck_gradients", ("keep_neck_activations", "keep_backbone_activations", "keep_full_activations"), "the activations of the neck do not survive the forward"),
              "backbone": ("backbone_gradients", ("keep_backbone_activations", "keep_full_activations"),
                           "the plan fuses convs of the backbone into other kernels and their activations do not survive the forward"),
              "full": ("full_gradients", ("keep_full_activations",),
                       "the plan fuses convs of the backbone into other kernels and their activations do not survive the forward")}

    def gradients(self, frames_or_x, bndbox, scope=None):
        """``(loss, {head_conv_layer: (dW, db)}, {conv_layer: dW [Cout,Cin,k,k]})`` over the BatchNorm convs of ``scope`` ("blocks",
        "neck", "backbone" or "full"; default ``self.trainable``): ``head_gradients``, then ``_walk`` through ``_graph(scope)``.  All on the
        current stream, nothing synchronises.  The model's ``options`` must hold ``keep_head_inputs`` and the option of the scope."""
        return self.batchnorm_gradients(frames_or_x, bndbox, scope)[:3]

    def batchnorm_gradients(self, frames_or_x, bndbox, scope=None):
        """``gradients`` with a fourth element: ``(loss, head grads, {conv_layer: dW}, {conv_layer: (dgamma [Cout], dbeta [Cout])})``.
        In batch mode (the model in ``.train()``, ``options['keep_bn_inputs']``) these are what ``loss.backward()`` of the reference's
        trainer leaves on ``conv.weight``, ``bn.weight`` and ``bn.bias`` of every BatchNorm conv of ``scope``: the walk turns the
        gradient of each BatchNorm output into that of the raw conv output by ``bn_grad_async`` over ``Darknet.read_bn_input`` and the
        plan's own statistics, and the conv gradients take no frozen scale.  On an eval model the fourth element is empty."""
        scope = self.trainable if scope is None else scope
        if scope not in self.SCOPES:
            raise ValueError("DarknetTrainer.gradients: scope must be 'blocks', 'neck', 'backbone' or 'full', got %r" % (scope,))
        self._require_bn_option("DarknetTrainer.gradients", scope)
        entry, kept, lost = self.SCOPES[scope]
        opts = getattr(self.darknet, "options", {})
        if not (int(opts.get("keep_head_inputs", 0)) and any(int(opts.get(name, 0)) for name in kept)):
            raise RuntimeError("DarknetTrainer.%s: set model.options['keep_head_inputs'] = 1 and model.options['%s'] = 1 before the first forward; "
                               "without them %s" % (entry, kept[0], lost))
        loss, head_grads, operands = self._head_pass(frames_or_x, bndbox)
        bn_grads = {} if self._batch_mode() else None
        return loss, head_grads, self._walk(loss, head_grads, operands, self._graph(scope), self._net_input, bn_grads), bn_grads or {}

    def block_gradients(self, frames_or_x, bndbox):
        """``(loss, {head_conv_layer: (dW, db)}, {block_conv_layer: dW [Cout,Cin,k,k]})``: what ``loss.backward()`` of the reference
        under ``.eval()`` leaves on the head convs and on ``conv.weight`` of the detection blocks (``Darknet.head_blocks``: the
        BatchNorm conv each head conv reads; BatchNorm frozen, its parameters are not trained).  ``head_gradients``, then the walk of
        ``neck_gradients`` over the heads and their blocks alone: per head with a block the data gradient from the head's float32
        master weights, the mask of the block conv's stored output (whose sign gives the leaky-ReLU derivative) fused into it, and
        rtod_conv_wgrad over ``read_layer`` of the block's input with the plan's frozen scale.  All on the current stream, nothing
        synchronises.  The model's ``options`` must hold ``keep_head_inputs`` and ``keep_block_inputs``."""
        return self.gradients(frames_or_x, bndbox, "blocks")

    def neck_gradients(self, frames_or_x, bndbox):
        """``(loss, {head_conv_layer: (dW, db)}, {neck_conv_layer: dW [Cout,Cin,k,k]})``: what ``loss.backward()`` of the reference
        under ``.eval()`` leaves on the head convs and on ``conv.weight`` of every neck conv (``Darknet.neck_layers``: the BatchNorm
        convs behind the backbone; BatchNorm frozen).  ``head_gradients``, then a walk through the neck graph in descending layer
        order that keeps the gradient with respect to each layer's OUTPUT:

        * a conv with ``dz`` (its output gradient times the mask of its own activation): ``dW`` by rtod_conv_wgrad over
          ``read_layer`` of its input with the plan's frozen scale, and, where its input is a neck layer, rtod_conv_dgrad from the
          float32 masters and that scale; the conv at the boundary of the graph gets a ``dW`` and sends nothing further;
        * a route hands each source its channel range; an upsample calls rtod_upsample2x_grad;
        * a producer with ONE reader inside the graph has its mask fused into that reader's call; one with several readers (or a
          route as its reader) gets the plain contributions, added in ascending reader order with float32 adds, then one
          multiplication by the mask.  Either way an element is chain(s), adds in a fixed order, one multiplication: bit-identical
          from call to call.

        All on the current stream, nothing synchronises.  The model's ``options`` must hold ``keep_head_inputs`` and
        ``keep_neck_activations`` (or ``keep_backbone_activations``, which keeps a superset)."""
        return self.gradients(frames_or_x, bndbox, "neck")

    def backbone_gradients(self, frames_or_x, bndbox):
        """``(loss, {head_conv_layer: (dW, db)}, {conv_layer: dW [Cout,Cin,k,k]})`` over ``Darknet.trainable_layers()``: the walk of
        ``neck_gradients`` carried on through the backbone, with two more kinds of layer.  A 3x3 / stride-2 conv calls
        rtod_conv_wgrad_s2 and rtod_conv_dgrad_s2.  A ``[shortcut]`` hands the gradient of its output to both sources unchanged; it
        carries no mask of its own, and a leaky conv that it alone reads has its mask applied by rtod_grad_join with that one
        contribution.  Layer 0 is not trained: the walk ends at the first layer whose input is outside the graph.  All
        on the current stream, nothing synchronises.  The model's ``options`` must hold ``keep_head_inputs`` and
        ``keep_backbone_activations``."""
        return self.gradients(frames_or_x, bndbox, "backbone")

    def full_gradients(self, frames_or_x, bndbox):
        """``(loss, {head_conv_layer: (dW, db)}, {conv_layer: dW [Cout,Cin,k,k]})`` over ``Darknet.full_layers()``: the walk of
        ``backbone_gradients`` with two more kinds of layer.  A conv whose ``Cin`` is no multiple of 32 calls rtod_conv_wgrad_thin
        and rtod_conv_dgrad_thin; layer 0 takes its ``dW`` over the prepared network input and sends nothing further.  A size-2
        ``[maxpool]`` calls rtod_maxpool_grad with ``read_layer`` of its input, which serves the winners and, where the pool is
        the one reader of a leaky conv, that conv's mask.  On YOLOv3-tiny this is every BatchNorm conv, what the reference's
        ``optim.Adam(self.darknet.parameters())`` trains with BatchNorm frozen.  All on the current stream, nothing synchronises.
        The model's ``options`` must hold ``keep_head_inputs`` and ``keep_full_activations``."""
        return self.gradients(frames_or_x, bndbox, "full")

    def _walk(self, loss, head_grads, operands, graph, net_input=None, bn_grads=None):
        """The one walk under ``gradients``: ``{conv_layer: dW}`` of the BatchNorm convs of ``graph = (layers, readers, member,
        scales)``, in descending layer order, from the heads' ``operands`` (``_head_pass``).  No layer is copied twice in one call:
        ``stored`` starts out with the head-conv inputs ``_head_pass`` read.  A layer's dense ``read_layer`` copy is dropped once the
        walk has passed the layer (every use of it lies at or behind it), and its entry of ``parts`` when its gradient is taken.
        ``bn_grads`` (a dict, batch mode): the gradient of a BatchNorm conv's output goes through ``bn_grad_async`` first — the raw conv
        output of the forward, the plan's statistics, the gamma master —, which leaves ``(dgamma, dbeta)`` there; the scales are None."""
        model = self.darknet
        layers, readers, member, scales = graph
        masters = self._masters(list(head_grads) + sorted(scales), loss.device)
        B = next(iter(operands.values()))[0].size(0)
        stored = {head - 1: x for head, (_, x) in operands.items()}
        if net_input is not None:
            stored[-1] = net_input.to(torch.float32).contiguous()     # what layer 0 read: no read_layer(-1)

        def read(layer):                                              # dense copies, one per layer and call
            if layer not in stored:
                stored[layer] = model.read_layer(layer, B)
            return stored[layer]

        parts = {}                                                    # producer -> [(reader, contribution)], or the finished gradient

        def send(producer, reader, contribution, fusable):
            """``contribution(y, slope)`` of ``reader`` to the output gradient of ``producer``."""
            if not member[producer]:
                return
            P = layers[producer]
            leaky = P.type == "convolutional" and P.leaky
            if fusable and leaky and sum(member[r] for r in readers[producer]) == 1:
                parts[producer] = contribution(read(producer), 0.1)
            else:
                parts.setdefault(producer, []).append((reader, contribution(None, 1.0)))

        def gradient(layer):
            """The gradient with respect to the layer's output; for a conv, times the mask of its activation."""
            got = parts.pop(layer)
            if not isinstance(got, list):
                return got
            got.sort(key=lambda rc: rc[0])
            L = layers[layer]
            leaky = L.type == "convolutional" and L.leaky
            if len(got) == 1 and not leaky:
                return got[0][1]
            return grad_join_async([c for _, c in got], read(layer) if leaky else None, 0.1 if leaky else 1.0)

        grads = {}
        for i in range(len(layers) - 1, -1, -1):
            if not member[i]:
                continue
            L = layers[i]
            if L.type == "convolutional":
                head = i in operands
                dz = operands[i][0] if head else gradient(i)
                scale = None if head else scales[i]
                if bn_grads is not None and not head:                 # du -> dz through the BatchNorm of the batch
                    dz, dgamma, dbeta = bn_grad_async(dz, model.read_bn_input(i, B), *model.bn_stats_dev(i), masters[i][2])
                    bn_grads[i] = (dgamma, dbeta)
                if not head and self.wgrad_precision == "f16s3" and L.stride == 1 and L.size in WGRAD_SPLIT_SIZES and conv_wgrad_split_takes(L.cin, L.size):
                    grads[i] = conv_wgrad_split_async(dz, read(i - 1), L.size, row_scale=scale)
                elif not head:
                    grads[i] = conv_wgrad_async(dz, read(i - 1), L.size, row_scale=scale, stride=L.stride)[0]
                if i > 0:
                    hw = (layers[i - 1].hout, layers[i - 1].wout)
                    if self.grad_precision == "f16s3" and L.size in GRAD_SPLIT_SIZES and conv_dgrad_split_takes(L.cin, L.size, L.stride):
                        send(i - 1, i, lambda y, slope, dz=dz, scale=scale, L=L: conv_dgrad_split_async(masters[i][0], dz, L.size, scale, y, slope), True)
                    else:
                        send(i - 1, i, lambda y, slope, dz=dz, scale=scale, L=L, hw=hw: conv_dgrad_async(masters[i][0], dz, L.size, scale, y, slope, L.stride, hw), True)
            elif L.type == "upsample":
                g = gradient(i)
                send(i - 1, i, lambda y, slope, g=g, L=L: upsample2x_grad_async(g, y, slope, "nearest" if L.nearest else "bilinear"), True)
            elif L.type == "maxpool":                                 # the pool's input copy gives the winners and the producer's mask
                g = gradient(i)
                send(i - 1, i, lambda y, slope, g=g, L=L, i=i: maxpool_grad_async(g, read(i - 1), slope, L.size, L.stride), True)
            elif L.type == "shortcut":                                # both sources take the gradient as it is
                g = gradient(i)
                for s in L.srcs:
                    send(s, i, lambda y, slope, g=g: g if y is None else grad_join_async([g], y, slope), True)
            else:                                                     # route: every source takes its channel range
                g, off = gradient(i), 0
                for s in L.srcs:
                    send(s, i, lambda y, slope, g=g, off=off, s=s: g.narrow(1, off, layers[s].cout).contiguous(), False)
                    off += layers[s].cout
            for k in [k for k in stored if k >= i]:                   # every use of layer k's copy lies at or behind layer k
                del stored[k]
        return {layer: grads[layer] for layer in sorted(grads)}

    def _graph(self, scope):
        """``(IR layers, readers per layer, membership per layer, {conv: device address of its frozen scale})`` of the graph ``_walk``
        goes through for ``scope``, asked of the plan once per plan and weight load.  The plan decides which BatchNorm convs belong
        (``Darknet.head_blocks`` / ``neck_layers`` / ``trainable_layers``).  "blocks": they and the head convs are the graph.  "neck"
        "backbone" and "full": routes, upsamples, in the trainable graph shortcuts and in the full graph size-2 max-pools follow by
        the plan's closure rule: every reader is a member or a [yolo] layer."""
        model = self.darknet
        key = (scope, model._plan.value, model._plan_weights_version, self._batch_mode())
        if self._graph_cache is None or self._graph_cache[0] != key:
            h = int(model.net_info["height"])
            w = int(model.input_width) if getattr(model, "input_width", None) is not None else h
            layers = build_ir(model.blocks, h, w).layers
            readers = [[] for _ in layers]
            for L in layers:
                for s in (L.srcs if L.type in ("route", "shortcut") else ((L.index - 1,) if L.index > 0 else ())):
                    readers[s].append(L.index)
            if scope == "blocks":
                trained = [block for _, block, _ in model.head_blocks() if block >= 0]
            else:
                trained = [conv for conv, _ in (model.neck_layers() if scope == "neck" else model.full_layers() if scope == "full" else model.trainable_layers())]
            convs = set(trained) | {c for c, _ in model.head_layers()}
            passive = {"blocks": (), "neck": ("route", "upsample"), "backbone": ("route", "upsample", "shortcut"),
                       "full": ("route", "upsample", "shortcut", "maxpool")}[scope]
            member = [False] * len(layers)
            for L in reversed(layers):
                ok = L.index in convs if L.type == "convolutional" else L.type in passive and bool(readers[L.index])
                if L.type == "maxpool":                               # rtod_maxpool_grad's pools (the plan's rule)
                    ok = ok and L.size == 2 and L.stride in (1, 2) and not L.pool_pad
                member[L.index] = ok and (scope == "blocks" or all(layers[r].type == "yolo" or member[r] for r in readers[L.index]))
            scales = {c: None if self._batch_mode() else model.conv_scale(c)[0] for c in trained}     # batch mode: nothing is folded
            self._graph_cache = (key, (layers, readers, member, scales))
        return self._graph_cache[1]

    # ------------------------------------------------------------------ the reference's training step, on the heads
    def feed_forward_through_model(self, batch_data, bndbox):
        """The reference's training step (train.py:412-425) with the backbone frozen: forward under ``train_mode()``, loss, the
        heads' gradients (``head_gradients``) and one ``optimizer`` step per head conv (``Darknet.step_conv``: masters, moments
        and the packed weights updated by one kernel each).  Everything is enqueued on the current stream and nothing
        synchronises; the next forward on that stream runs the new weights.  Returns the loss from before the step as a 0-dim
        float32 device tensor.  The module's ``conv.weight`` / ``conv.bias`` lag behind until ``sync_parameters()`` (or anything
        that reads the model's parameters as a whole: ``weight_stream()``, ``state_dict()``, a re-pack)."""
        if self.trainable in self.SCOPES:
            # every gradient kernel of the batch is enqueued before the first step, as autograd has it: the steps update the
            # masters in place, and the data gradients through the heads and the neck convs read them
            loss, grads, block_grads, bn_grads = self.batchnorm_gradients(batch_data, bndbox)
            grads = dict(grads)
            for layer, dw in block_grads.items():
                grads[layer] = _slots(conv_kind(self.darknet, layer), dict(zip(("gamma", "beta"), bn_grads.get(layer, ())), weight=dw))
        else:
            loss, grads = self.head_gradients(batch_data, bndbox)
        self.optimizer.step(self.darknet, self._masters(grads, loss.device), grads)
        return loss

    def sync_parameters(self):
        """Copy the masters into the module's ``conv.weight`` / ``conv.bias`` (one synchronisation).  The plan already runs these
        weights, so it is not invalidated: no re-pack follows."""
        self.darknet.sync_stepped_parameters()
