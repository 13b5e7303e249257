#!/usr/bin/env python
"""What training ALL of YOLOv3-tiny (every conv of Darknet.full_layers: through the max-pools, layer 0 included) costs in a training
step, in ONE process (fp32, synthetic weights, seeded frames and boxes):

    python tools/exp_full_grad.py [--res 416] [--batch 8] [--ubench tools/ubench_launch] [--log profiles/experiments/full_grad_cost.log]

each path on a model of its own:
  (a) forward under train_mode() on a default plan              the yardstick "one forward"
  (b) the same on a plan with keep_full_activations             what the option costs the forward
  (c) feed_forward_through_model, trainable="neck"              forward + heads + the five neck convs: the path as it was
  (d) feed_forward_through_model, trainable="full"              forward + heads + all 11 BatchNorm convs
and, alone on the operands of one recorded walk of (d):
  maxpool_grad     rtod_maxpool_grad, the six pools
  wgrad_thin_0/2   rtod_conv_wgrad_thin of layer 0 (Cin 3) and layer 2 (Cin 16): slice kernel + tree reduce
  dgrad_thin_2     rtod_conv_dgrad_thin of layer 2 (the gradient with respect to pool 1's output)
Beside each thin wgrad stands the time to read its dz and x ONCE at the streaming rate tools/ubench_launch measures on the same box
("read 47 MB"; the binary is run as a child process before this process touches the GPU; without it the floor is left out).
Alternating rounds, HIP events around windows of --iters calls, medians.  The learning rate is tiny (1e-9).  Nothing here gates a speed."""
import argparse, json, os, re, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--ubench", default=os.path.join("tools", "ubench_launch"), help="the built tools/ubench_launch.hip")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "full_grad_cost.log"))
args = ap.parse_args()

stream_gbps = None
if os.path.isfile(args.ubench) and os.access(args.ubench, os.X_OK):
    out = subprocess.run([os.path.abspath(args.ubench)], capture_output=True, text=True, timeout=120).stdout
    hit = re.search(r"^read 47 MB\s+([0-9.]+) us per launch", out, re.M)
    if hit:
        stream_gbps = 47 * 1024 * 1024 / float(hit.group(1)) / 1e3     # bytes per us -> GB/s

import grad_walk
import torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir

assert torch.cuda.is_available(), "exp_full_grad.py measures on the GPU"
LR = 1e-9
events = lambda fn: grad_walk.events(fn, args.iters)
trainer = lambda trainable, options: grad_walk.trainer(cfg_text, ir, args.res, "fp32", trainable, options, LR)

x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)
NECK = {"keep_head_inputs": 1, "keep_neck_activations": 1}
FULL = {"keep_head_inputs": 1, "keep_full_activations": 1}
cfg_text = cfgs.yolov3_tiny_cfg(args.res, args.res)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
ta, tb, tn, tc = trainer("heads", {}), trainer("heads", FULL), trainer("neck", NECK), trainer("full", FULL)
fns = [lambda: ta._forward_train(x), lambda: tb._forward_train(x), lambda: tn.feed_forward_through_model(x, targets), lambda: tc.feed_forward_through_model(x, targets)]
for f in fns:
    events(f)                                                     # warm-up of every shape the timed windows use
m = tc.darknet
calls, grads = grad_walk.record(tc, x, targets, "full_gradients")
replay = lambda group: (lambda: [f(*a, **k) for f, a, k in group])
cin_of = lambda c: int(c[1][1].size(1))                           # wgrad: (dz, x, size, ...); dgrad: (w, dz, size, ...): Cin is dim 1 of the second / first
thin_w = {cin_of(c): c for c in calls["wgrad"] if cin_of(c) % 32}
thin_d = [c for c in calls["dgrad"] if int(c[1][0].size(1)) % 32]
assert sorted(thin_w) == [3, 16] and len(thin_d) == 1 and len(calls["maxpool_grad"]) == 6 and len(grads) == 11
groups = {"maxpool_grad": calls["maxpool_grad"], "wgrad_thin_0": [thin_w[3]], "wgrad_thin_2": [thin_w[16]], "dgrad_thin_2": thin_d,
          "wgrad_all": calls["wgrad"], "dgrad_all": calls["dgrad"], "read_layer": calls["read_layer"]}
fns += [replay(g) for g in groups.values()]
for f in fns[4:]:
    events(f)
times = [[] for _ in fns]
for r in range(args.rounds):
    for t, f in zip(times, fns):
        t.append(events(f))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
keys = ["forward_default", "forward_option", "neck_step", "full_step"] + list(groups)
us = dict(zip(keys, [statistics.median(t) for t in times]))
floor = {}
for name, c in (("wgrad_thin_0", thin_w[3]), ("wgrad_thin_2", thin_w[16])):
    dz, xx, size = c[1][0], c[1][1], int(c[1][2])
    nbytes = 4 * (dz.numel() + xx.numel())
    S, L = grad_walk.T.conv_wgrad_thin_slices(dz.size(0), dz.size(1), xx.size(1), xx.size(2), xx.size(3), size)
    floor[name] = {"bytes_dz_and_x": nbytes, "slices": S, "slice_len": L, "us": round(us[name], 1),
                   "read_once_us": None if stream_gbps is None else round(nbytes / stream_gbps / 1e3, 1),
                   "over_floor": None if stream_gbps is None else round(us[name] / (nbytes / stream_gbps / 1e3), 2)}
res = {"net": "yolov3-tiny", "res": args.res, "batch": args.batch, "precision": m.active_precision, "boxes_per_image": args.boxes,
       "full_convs": len(grads), "full_weights": int(sum(dw.numel() for dw in grads.values())), "loss": float(tc.last_components[0].item()), "status": int(tc.status.item()),
       "us": {k: round(v, 1) for k, v in us.items()},
       "option_over_forward": round(us["forward_option"] / us["forward_default"], 3),
       "full_step_over_forward": round(us["full_step"] / us["forward_default"], 2), "full_step_over_neck_step": round(us["full_step"] / us["neck_step"], 2),
       "calls": {g: len(c) for g, c in groups.items()},
       "stream_read_gbps": None if stream_gbps is None else round(stream_gbps, 1), "thin_wgrad_against_one_read": floor,
       "arena_bytes": {"default": int(ta.darknet._info.arena_bytes), "neck": int(tn.darknet._info.arena_bytes), "full": int(m._info.arena_bytes)},
       "spread_us": dict(zip(keys, [round(max(t) - min(t), 1) for t in times]))}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
