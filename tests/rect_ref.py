"""CPU reference of a rectangular forward (test helper).

``oracle.darknet_ref.RefDarknet(cfg, h, w)`` resolves a rectangular trunk, but its ``predict_transform`` reshapes a head to
``G*G`` and so only decodes square grids.  ``forward_rect`` walks the same ``RefDarknet.ir`` / ``.params`` layer by layer with
the same PyTorch CPU ops as ``RefDarknet.forward`` and decodes each head with the reference's arithmetic (src/util.py:193-237)
generalised to a ``GH x GW`` grid: one stride ``height // GH`` (== ``width // GW``), rows ``r = (gy * GW + gx) * A + a``.
For ``h == w`` it reproduces ``RefDarknet.forward`` bit for bit (tests/test_rect_host.py checks that).
"""
import torch
import torch.nn.functional as F


def predict_transform_rect(prediction, height, anchors, num_class, train=False):
    B, GH, GW = prediction.size(0), prediction.size(2), prediction.size(3)
    stride = height // GH
    attrs = 5 + num_class
    A = len(anchors)
    p = prediction.reshape(B, attrs * A, GH * GW).transpose(1, 2).contiguous().view(B, GH * GW * A, attrs)
    p = p.clone()
    p[:, :, 0] = torch.sigmoid(p[:, :, 0])
    p[:, :, 1] = torch.sigmoid(p[:, :, 1])
    p[:, :, 4:] = torch.sigmoid(p[:, :, 4:])
    if not train:
        anc = torch.FloatTensor([(a[0] / stride, a[1] / stride) for a in anchors])
        gy, gx = torch.meshgrid(torch.arange(GH), torch.arange(GW), indexing="ij")
        off = torch.stack((gx.reshape(-1), gy.reshape(-1)), 1)          # [GH*GW, 2] (x, y)
        off = off.repeat(1, A).view(-1, 2).unsqueeze(0)                  # [1, GH*GW*A, 2]
        p[:, :, :2] += off
        p[:, :, 2:4] = torch.exp(p[:, :, 2:4]) * anc.repeat(GH * GW, 1).unsqueeze(0)
        p[:, :, :4] *= stride
    return p


def predict_transform_v5_rect(prediction, height, anchors, num_class):
    """oracle.darknet_ref.predict_transform_v5 (cfg extension decode=v5) on a GH x GW grid."""
    B, GH, GW = prediction.size(0), prediction.size(2), prediction.size(3)
    stride = height // GH
    attrs, A = 5 + num_class, len(anchors)
    p = prediction.reshape(B, attrs * A, GH * GW).transpose(1, 2).contiguous().view(B, GH * GW * A, attrs)
    y = torch.sigmoid(p)
    gy, gx = torch.meshgrid(torch.arange(GH), torch.arange(GW), indexing="ij")
    off = torch.stack((gx.reshape(-1), gy.reshape(-1)), 1).repeat(1, A).view(-1, 2).unsqueeze(0).float()
    anc = torch.FloatTensor([(float(a[0]), float(a[1])) for a in anchors]).repeat(GH * GW, 1).unsqueeze(0)
    out = y.clone()
    out[:, :, 0:2] = (y[:, :, 0:2] * 2.0 - 0.5 + off) * stride
    out[:, :, 2:4] = (y[:, :, 2:4] * 2) ** 2 * anc
    return out


def forward_rect(ref, x, keep_layers=False):
    """``ref``: an ``oracle.darknet_ref.RefDarknet`` built for ``(height, width)`` with weights loaded; ``x`` float32
    ``[B,3,height,width]`` -> ``[B,N,5+C]`` (eval BatchNorm), and the per-layer outputs with ``keep_layers``."""
    outputs = {}
    detections = None
    for L in ref.ir.layers:
        i = L.index
        if L.type == "convolutional":
            p = ref.params[i]
            x = F.conv2d(x, p["weight"], p.get("bias"), L.stride, L.pad)
            if L.bn:
                x = F.batch_norm(x, p["mean"], p["var"], p["gamma"], p["beta"], training=False, momentum=0.1, eps=1e-5)
            if L.leaky:
                x = F.leaky_relu(x, 0.1)
            elif L.silu:
                x = F.silu(x)
        elif L.type == "upsample":
            if L.nearest:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        elif L.type == "maxpool":
            if L.pool_pad:
                x = F.max_pool2d(x, L.size, L.stride, L.pool_pad)
            elif L.stride != 1:
                x = F.max_pool2d(x, L.size, L.stride)
            else:
                x = F.pad(x, (0, L.size - 1, 0, L.size - 1), mode="replicate")
                x = F.max_pool2d(x, L.size, L.size - 1)
        elif L.type == "shortcut":
            x = outputs[L.srcs[0]] + outputs[L.srcs[1]]
        elif L.type == "route":
            x = outputs[L.srcs[0]] if len(L.srcs) == 1 else torch.cat([outputs[s] for s in L.srcs], 1)
        elif L.type == "yolo":
            x = (predict_transform_v5_rect if L.decode_v5 else predict_transform_rect)(x, ref.height, L.anchors, L.classes)
            detections = x if detections is None else torch.cat((detections, x), 1)
            outputs[i] = outputs[i - 1]
            continue
        outputs[i] = x
    if keep_layers:
        return detections, outputs
    return detections


def synth_frames_rect(batch, height, width, seed):
    """``x ~ U[0,1)`` float32 ``[B,3,height,width]`` (synth.synth_frames' distribution, rectangular)."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random((batch, 3, height, width), dtype=np.float32)
