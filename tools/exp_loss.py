#!/usr/bin/env python
"""What the reference's training loss costs on top of a forward, in ONE process (synthetic weights, seeded frames and boxes):

    python tools/exp_loss.py [--net yolov3] [--res 416] [--batch 8] [--log profiles/experiments/loss_cost.log]

  write_results_async alone                                                    (the yardstick, as for the validator)
  forward under train_mode()                                                   against
  forward + loss_from_boxes                                                    (the fused route: no dense target)
  forward + loss_from_boxes + finish_decode + write_results_async              (what validate_model(loss=True) runs per batch)
  forward + target_creator + darknet_loss                                      (the dense route, the reference's call sequence)
Alternating rounds, HIP events, medians.  The boxes are CocoTargets-like rows: a dozen per image, most of class 0, a few small."""
import argparse, json, os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.train import DarknetTrainer
from realtimeobjectdetection_amd.util import write_results_async

ap = argparse.ArgumentParser()
ap.add_argument("--net", default="yolov3"); ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--conf", type=float, default=0.6); ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "loss_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_loss.py measures on the GPU"

cfg_text = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg}[args.net](args.res, args.res)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
with tempfile.TemporaryDirectory() as d:
    m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
    m.net_info["height"] = args.res
    m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
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
trainer = DarknetTrainer(m)
with torch.no_grad():
    y = m(x)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3                 # us per call


def nms_only():
    write_results_async(y, 80, args.conf, 0.5)


def forward():
    with torch.no_grad(), m.train_mode():
        return m(x)


def forward_loss():
    pred = forward()
    trainer.loss_from_boxes(pred, targets)
    return pred


def forward_loss_detect():
    write_results_async(m.finish_decode(forward_loss()), 80, args.conf, 0.5)


def forward_dense():
    pred = forward()
    target, mask = trainer.target_creator(targets)
    trainer.darknet_loss(pred, target, mask)


fns = (nms_only, forward, forward_loss, forward_loss_detect, forward_dense)
for f in fns:
    events(f)                                                     # warm-up of every shape the timed windows use
times = [[] for _ in fns]
for _ in range(args.rounds):
    for t, f in zip(times, fns):
        t.append(events(f))
med = [statistics.median(t) for t in times]
loss, comp = trainer.loss_from_boxes(forward(), targets)
res = {"net": args.net, "res": args.res, "batch": args.batch, "precision": m.active_precision, "boxes_per_image": args.boxes,
       "loss": float(comp[0].item()), "status": int(trainer.status.item()),
       "write_results_us": round(med[0], 1), "forward_us": round(med[1], 1), "forward_loss_us": round(med[2], 1),
       "forward_loss_finish_write_results_us": round(med[3], 1), "forward_target_creator_darknet_loss_us": round(med[4], 1),
       "loss_cost_us": round(med[2] - med[1], 1), "dense_route_cost_us": round(med[4] - med[1], 1),
       "spread_us": [round(max(t) - min(t), 1) for t in times]}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
