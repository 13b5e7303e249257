"""Host-side mirror of the hot-path half of the reference's ``src/util.py`` on librtod.so.

Same names, argument meaning and return conventions as the reference (SURVEY.md §8 b):

* ``predict_transform(prediction, inp_dim, anchors, num_class, CUDA, TRAIN=False)``  src/util.py:175-239
* ``write_results(prediction, num_class, confidence=0.6, nms_conf=0.4)``              src/util.py:242-346
  -> float32 ``[D,8]`` tensor on prediction's device, or the Python int ``0``
* ``confidence_mask(tensor, confidence)``                                              src/util.py:106-117
* ``bbox_iou(box1, box2)``                                                             src/util.py:120-153
* ``prep_image`` / ``rescale_boxes`` (int or ``(width, height)`` canvas), ``prep_frames`` (batched, new)    src/util.py:349-397

All tensors must be CUDA (ROCm) float32 tensors; there is no CPU fallback.
"""
import ctypes as C

import torch

from . import _ffi

COCO_NAMES = ("person bicycle car motorbike aeroplane bus train truck boat|traffic light|fire hydrant|stop sign|parking meter|bench "
              "bird cat dog horse sheep cow elephant bear zebra giraffe backpack umbrella handbag tie suitcase frisbee skis snowboard|"
              "sports ball|kite|baseball bat|baseball glove|skateboard surfboard|tennis racket|bottle|wine glass|cup fork knife spoon bowl "
              "banana apple sandwich orange broccoli carrot|hot dog|pizza donut cake chair sofa pottedplant bed diningtable toilet "
              "tvmonitor laptop mouse remote keyboard|cell phone|microwave oven toaster sink refrigerator book clock vase scissors|"
              "teddy bear|hair drier|toothbrush")


def load_classes(names_file_path: str = None) -> list:
    """Class labels (reference: src/util.py:400-411 reads data/coco.names).  Without a file the 80 COCO names
    of the Darknet distribution are returned."""
    if names_file_path:
        with open(names_file_path, "r") as fp:
            return fp.read().split("\n")[:-1]
    out = []
    for chunk in COCO_NAMES.split("|"):
        chunk = chunk.strip()
        if " " in chunk and chunk in ("traffic light", "fire hydrant", "stop sign", "parking meter", "sports ball", "baseball bat",
                                      "baseball glove", "tennis racket", "wine glass", "hot dog", "cell phone", "teddy bear",
                                      "hair drier"):
            out.append(chunk)
        else:
            out.extend(chunk.split())
    return out


def _canvas(inp_dim):
    """``inp_dim`` -> (width, height): an int is the reference's square canvas, a pair is ``letterbox_image``'s (w, h)."""
    if isinstance(inp_dim, (tuple, list)):
        if len(inp_dim) != 2:
            raise ValueError("inp_dim: expected an int or a (width, height) pair, got %r" % (inp_dim,))
        return int(inp_dim[0]), int(inp_dim[1])
    return int(inp_dim), int(inp_dim)


def letterbox_geometry(img_w: int, img_h: int, size) -> tuple:
    """``(new_w, new_h, off_x, off_y)`` of ``letterbox_image(img, (w, h))`` (reference: src/util.py:360-370: Python float
    ``min``, ``int()`` truncation, ``// 2`` offsets) for a canvas ``size`` = int or (width, height): what the prep kernels place
    and what ``rescale_boxes`` undoes.  Host arithmetic only."""
    w, h = _canvas(size)
    s = min(w / img_w, h / img_h)
    new_w, new_h = int(img_w * s), int(img_h * s)
    return new_w, new_h, (w - new_w) // 2, (h - new_h) // 2


def prep_image(img, inp_dim, mode="BGR", device=None) -> torch.Tensor:
    """uint8 HWC image (numpy or torch) -> float32 ``[1,3,inp_dim,inp_dim]`` network input on the GPU
    (reference: src/util.py:375-397 + letterbox_image 349-372).  Only the uint8 pixels cross PCIe; resize,
    padding, channel swap and /255 run in a HIP kernel.  ``mode='BGR'`` (OpenCV order, the reference's default)
    is swapped to RGB.  Parity with cv2.INTER_CUBIC is unpinned (OpenCV is not available offline).
    ``inp_dim`` may also be a ``(width, height)`` pair (letterbox_image's convention): ``[1,3,height,width]``."""
    assert mode == "BGR" or mode == "RGB"
    t = torch.as_tensor(img)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.size(2) != 3:
        raise ValueError("prep_image: expected uint8 [H,W,3], got %s %s" % (t.dtype, tuple(t.shape)))
    if isinstance(inp_dim, (tuple, list)):
        return prep_frames(t.unsqueeze(0), inp_dim, mode=mode, device=device)
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = t.to(device).contiguous()
    out = torch.empty((1, 3, int(inp_dim), int(inp_dim)), dtype=torch.float32, device=t.device)
    _ffi.enqueue("rtod_prep_image", t.device, t, t.size(0), t.size(1), 1 if mode == "BGR" else 0, int(inp_dim), out)
    return out


def prep_frames(frames, size, mode="BGR", device=None) -> torch.Tensor:
    """uint8 ``[B,H,W,3]`` frames of one camera size (numpy or torch) -> float32 ``[B,3,height,width]`` on the GPU in one
    kernel launch, ``size = (width, height)`` or an int for a square canvas: ``prep_image`` of every frame, letterboxed
    exactly like ``letterbox_image(img, (width, height))`` (rtod_prep_frames)."""
    assert mode == "BGR" or mode == "RGB"
    w, h = _canvas(size)
    t = torch.as_tensor(frames)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.size(3) != 3 or t.size(0) < 1:
        raise ValueError("prep_frames: expected uint8 [B,H,W,3], got %s %s" % (t.dtype, tuple(t.shape)))
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = t.to(device).contiguous()
    out = torch.empty((t.size(0), 3, h, w), dtype=torch.float32, device=t.device)
    _ffi.enqueue("rtod_prep_frames", t.device, t, t.size(0), t.size(1), t.size(2), 1 if mode == "BGR" else 0, h, w, out)
    return out


def rescale_boxes(output: torch.Tensor, im_dim_list: torch.Tensor, inp_dim) -> torch.Tensor:
    """Undo the letterbox on detection rows ``[img,x1,y1,x2,y2,...]`` and clamp to the image
    (reference: detect.py:120-136, which hard-codes 416 for the scale; here the actual ``inp_dim``).
    ``im_dim_list``: ``[n_images, 2]`` = (width, height) per image.  ``inp_dim``: int, or the ``(width, height)`` of a
    rectangular canvas (offsets ``(w - s*img_w)/2`` and ``(h - s*img_h)/2`` per axis).  Returns a new tensor."""
    out = output.clone()
    cw, ch = _canvas(inp_dim)
    dims = im_dim_list.to(out.device, torch.float32)[out[:, 0].long()]
    if cw == ch and not isinstance(inp_dim, (tuple, list)):
        scale = torch.min(float(inp_dim) / dims, 1)[0].view(-1, 1)
        out[:, [1, 3]] -= (inp_dim - scale * dims[:, 0].view(-1, 1)) / 2
        out[:, [2, 4]] -= (inp_dim - scale * dims[:, 1].view(-1, 1)) / 2
    else:
        canvas = torch.tensor([cw, ch], dtype=torch.float32, device=out.device)
        scale = torch.min(canvas / dims, 1)[0].view(-1, 1)
        out[:, [1, 3]] -= (cw - scale * dims[:, 0].view(-1, 1)) / 2
        out[:, [2, 4]] -= (ch - scale * dims[:, 1].view(-1, 1)) / 2
    out[:, 1:5] /= scale
    out[:, [1, 3]] = torch.minimum(torch.clamp(out[:, [1, 3]], min=0.0), dims[:, 0].view(-1, 1))
    out[:, [2, 4]] = torch.minimum(torch.clamp(out[:, [2, 4]], min=0.0), dims[:, 1].view(-1, 1))
    return out


def _need_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s: expected a CUDA (ROCm) tensor; this build has no CPU path" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s: expected float32, got %s" % (name, t.dtype))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def predict_transform(prediction, inp_dim, anchors, num_class, CUDA=True, TRAIN=False) -> torch.Tensor:
    _need_cuda(prediction, "predict_transform")
    if prediction.dim() != 4 or prediction.size(2) != prediction.size(3):
        raise ValueError("predict_transform: expected [B, A*(5+C), G, G], got %s" % (tuple(prediction.shape),))
    B, ch, G = prediction.size(0), prediction.size(1), prediction.size(2)
    attrs = 5 + int(num_class)
    A = len(anchors)
    if ch != A * attrs:
        raise ValueError("predict_transform: %d channels != %d anchors * %d attrs" % (ch, A, attrs))
    x = prediction.contiguous()
    out = torch.empty((B, G * G * A, attrs), dtype=torch.float32, device=x.device)
    anc = (C.c_float * (2 * A))(*[float(v) for a in anchors for v in a])
    _ffi.enqueue("rtod_predict_transform", x.device, x, B, attrs, G, A, anc, int(inp_dim), 1 if TRAIN else 0, out)
    return out


def confidence_mask(tensor: torch.Tensor, confidence: float) -> torch.Tensor:
    _need_cuda(tensor, "confidence_mask")
    if tensor.dim() != 3 or tensor.size(2) < 5:
        raise ValueError("confidence_mask: expected [B,N,>=5]")
    x = tensor.contiguous()
    out = torch.empty_like(x)
    _ffi.enqueue("rtod_confidence_mask", x.device, x, x.size(0) * x.size(1), x.size(2), float(confidence), out)
    return out


def bbox_iou(box1: torch.Tensor, box2: torch.Tensor) -> torch.Tensor:
    """IoU of one box against k boxes with the reference's +1 pixel convention."""
    _need_cuda(box1, "bbox_iou")
    _need_cuda(box2, "bbox_iou")
    b1 = box1.reshape(-1, box1.size(-1))
    b2 = box2.reshape(-1, box2.size(-1))
    if b1.size(0) != 1 or b1.size(1) < 4 or b2.size(1) < 4:
        raise NotImplementedError("bbox_iou: one box [1,>=4] against k boxes [k,>=4] (the reference's only use)")
    b1 = b1.contiguous()
    b2 = b2.contiguous()
    k = b2.size(0)
    out = torch.empty((k,), dtype=torch.float32, device=b2.device)
    _ffi.enqueue("rtod_bbox_iou", b2.device, b1, b2, k, b2.size(1), out)
    return out


_host_cache = {}


def _host_ints(dev):
    """Pinned int32[4] per device: landing place of write_results' counts and the split-f16 range flag."""
    h = _host_cache.get(dev.index)
    if h is None:
        h = _host_cache[dev.index] = torch.empty(4, dtype=torch.int32).pin_memory()
    return h


def _nms_buffers(dev, B, n, cap):
    """``(workspace, rows [cap,8], counts, workspace bytes)`` of write_results / nms_class_offset, kept together per shape (and
    stream) in ``_ffi.cache``."""
    def build():
        nbytes = C.c_size_t()
        _ffi.check(_ffi.lib().rtod_write_results_workspace(B, n, C.byref(nbytes)))
        ws = torch.empty((nbytes.value + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        out = torch.empty((max(cap, 1), 8), dtype=torch.float32, device=dev)
        counts = torch.zeros((2 + B + 2,), dtype=torch.int32, device=dev)
        return ws, out, counts, nbytes.value
    return _ffi.cache.get(_ffi.stream_key(dev) + ("nms_buffers", (B, n, cap)), build)


def write_results_async(prediction, num_class, confidence=0.6, nms_conf=0.4, cap=None):
    """Enqueue filter + NMS; returns device tensors ``(rows[cap,8], counts)`` without synchronising.

    ``counts[0]`` = D (valid rows; may exceed cap), ``counts[1]`` = candidates over the batch,
    ``counts[2:2+B]`` = detections per image.  The buffers are reused by the next call with the
    same shape: consume (or clone) them before calling again.
    """
    _need_cuda(prediction, "write_results")
    if prediction.dim() != 3 or prediction.size(2) != 5 + int(num_class):
        raise ValueError("write_results: expected [B,N,5+num_class], got %s" % (tuple(prediction.shape),))
    x = prediction.contiguous()
    B, n = x.size(0), x.size(1)
    if cap is None:
        cap = min(B * n, 16384)
    ws, out, counts, nbytes = _nms_buffers(x.device, B, n, int(cap))
    _ffi.enqueue("rtod_write_results", x.device, x, B, n, int(num_class), float(confidence), float(nms_conf), out, int(cap), counts, ws, nbytes)
    return out, counts


def nms_class_offset(prediction, num_class, conf_thres=0.25, iou_thres=0.45, max_wh=7680.0, max_det=300):
    """YOLOv5-style post-processing (NOT reference behaviour: the reference fetches its YOLOv5 model from the hub,
    detect.py:255-285; this follows the published class-offset batched NMS — parity unpinned).  ``prediction``
    ``[B,N,5+C]`` rows ``(cx,cy,w,h,obj,cls...)`` -> ``[D,8]`` rows ``[img,x1,y1,x2,y2,conf,obj,cls]``, per image by
    descending ``conf = obj * max cls`` (ties: lower row first), at most ``max_det`` per image; one host sync."""
    out, counts = nms_class_offset_async(prediction, num_class, conf_thres, iou_thres, max_wh, max_det)
    return out[:int(counts[0].item())].clone()


def nms_class_offset_async(prediction, num_class, conf_thres=0.25, iou_thres=0.45, max_wh=7680.0, max_det=300, cap=None):
    """nms_class_offset without the host synchronisation: device tensors ``(rows[cap,8], counts)``, ``counts[0]`` = valid rows
    (buffers are reused by the next call of the same shape, like write_results_async's)."""
    _need_cuda(prediction, "nms_class_offset")
    if prediction.dim() != 3 or prediction.size(2) != 5 + int(num_class):
        raise ValueError("nms_class_offset: expected [B,N,5+num_class], got %s" % (tuple(prediction.shape),))
    x = prediction.contiguous()
    B, n = x.size(0), x.size(1)
    if cap is None:
        cap = B * min(n, int(max_det))
    ws, out, counts, nbytes = _nms_buffers(x.device, B, n, int(cap))
    _ffi.enqueue("rtod_nms_class_offset", x.device, x, B, n, int(num_class), float(conf_thres), float(iou_thres), float(max_wh), int(max_det),
                 out, int(cap), counts, ws, nbytes)
    return out, counts


def write_results(prediction, num_class, confidence=0.6, nms_conf=0.4):
    """Reference-compatible: new ``[D,8]`` tensor, an empty ``[0,8]`` tensor when candidates existed
    but none had a non-zero class score (what the reference's concatenation yields), or int ``0``."""
    B, n = prediction.size(0), prediction.size(1)
    out, counts = write_results_async(prediction, num_class, confidence, nms_conf)
    from .darknet import take_pending_overflow, raise_overflow
    model, flag = take_pending_overflow(prediction)     # split-f16 range guard of the forward that produced `prediction`
    host = _host_ints(prediction.device)
    host[:2].copy_(counts[:2], non_blocking=True)
    if flag is not None:
        host[2:3].copy_(flag.reshape(-1)[:1], non_blocking=True)
    torch.cuda.current_stream(prediction.device).synchronize()   # ONE host sync (counts + flag), like the reference's own .tolist()/nonzero
    D, cand = int(host[0]), int(host[1])
    if flag is not None and int(host[2]) != 0:
        raise_overflow(model)
    if D > out.size(0):                        # more detections than the default capacity: redo at full size
        out, counts = write_results_async(prediction, num_class, confidence, nms_conf, cap=B * n)
        D = int(counts[0].item())
    if cand == 0:
        return 0
    return out[:D].clone()
