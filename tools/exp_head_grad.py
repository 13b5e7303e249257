#!/usr/bin/env python
"""What the gradients of the detection-head convs cost on top of a forward and its loss, in ONE process (synthetic weights, seeded
frames and boxes):

    python tools/exp_head_grad.py [--res 416] [--batch 8] [--log profiles/experiments/head_grad_cost.log]

for YOLOv3 (f16s3) and YOLOv3-tiny (fp32):
  forward under train_mode()                                    on a plan without option keep_head_inputs (the path as it was)
  forward + loss_from_boxes                                     on that plan
  forward + head_gradients                                      on a plan with keep_head_inputs: rtod_yolo_loss_grad, per head read_layer
                                                                of the conv's input + rtod_conv1x1_wgrad
Alternating rounds, HIP events, medians.  "head_grad_added_us" is forward + head_gradients minus forward + loss_from_boxes."""
import argparse, json, os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.train import DarknetTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "head_grad_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_head_grad.py measures on the GPU"


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3                 # us per call


def model(cfg_text, ir, precision, options):
    with tempfile.TemporaryDirectory() as d:
        m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
        m.net_info["height"] = args.res
        m.precision = precision
        m.options = dict(options)
        m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
    return m


x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
rng = np.random.default_rng(1)
targets = []
for b in range(args.batch):
    t = np.zeros((args.boxes, 85), np.float32)
    t[:, 0:2] = rng.uniform(1, args.res - 1, (args.boxes, 2))
    t[:, 2:4] = rng.uniform(12, args.res / 2, (args.boxes, 2))
    t[:, 4] = 1
    t[np.arange(args.boxes), 5 + rng.choice([0, 0, 0, 0, 16], args.boxes)] = 1
    targets.append(torch.from_numpy(t).cuda())

for net, make_cfg, precision in (("yolov3", cfgs.yolov3_cfg, "f16s3"), ("yolov3-tiny", cfgs.yolov3_tiny_cfg, "fp32")):
    cfg_text = make_cfg(args.res, args.res)
    ir = build_ir(parse_cfg_text(cfg_text), args.res)
    plain, kept = model(cfg_text, ir, precision, {}), model(cfg_text, ir, precision, {"keep_head_inputs": 1})
    t_plain, t_kept = DarknetTrainer(plain), DarknetTrainer(kept)

    def forward():
        with torch.no_grad(), plain.train_mode():
            return plain(x)

    def forward_loss():
        t_plain.loss_from_boxes(forward(), targets)

    def forward_head_gradients():
        t_kept.head_gradients(x, targets)

    fns = (forward, forward_loss, forward_head_gradients)
    for f in fns:
        events(f)                                                 # warm-up of every shape the timed windows use (autotune included)
    times = [[] for _ in fns]
    for _ in range(args.rounds):
        for t, f in zip(times, fns):
            t.append(events(f))
    med = [statistics.median(t) for t in times]
    loss, grads = t_kept.head_gradients(x, targets)
    gemm_flops = sum(2 * dw.numel() * args.batch * g[0] * g[1] for (dw, _), g in zip(grads.values(), t_kept.heads))
    res = {"net": net, "res": args.res, "batch": args.batch, "precision": kept.active_precision, "boxes_per_image": args.boxes,
           "loss": float(t_kept.last_components[0].item()), "status": int(t_kept.status.item()),
           "forward_us": round(med[0], 1), "forward_loss_us": round(med[1], 1), "forward_head_gradients_us": round(med[2], 1),
           "loss_cost_us": round(med[1] - med[0], 1), "head_grad_added_us": round(med[2] - med[1], 1),
           "wgrad_gflop": round(gemm_flops / 1e9, 2), "arena_bytes": [int(plain._info.arena_bytes), int(kept._info.arena_bytes)],
           "spread_us": [round(max(t) - min(t), 1) for t in times]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")
    del plain, kept, t_plain, t_kept
    torch.cuda.empty_cache()
