#!/usr/bin/env python
"""What the opt-in split-f16 data gradients (DarknetTrainer(grad_precision="f16s3"): rtod_conv_dgrad_split) change in a training
step, in ONE process (synthetic weights, seeded frames and boxes):

    python tools/exp_grad_split.py [--net yolov3|tiny] [--res 416] [--batch 8] [--log profiles/experiments/grad_split_cost.log]

YOLOv3 (f16s3, scope backbone; --net tiny: YOLOv3-tiny, scope full), each path on a model of its own:
  (a) forward under train_mode() on a default plan                            the yardstick "one forward"
  (b) feed_forward_through_model, grad_precision="fp32"                       the parent's exact step, re-measured here
  (c) feed_forward_through_model, grad_precision="f16s3"
and, on the operands of one recorded exact walk, the stride-1 data gradients the split ENTRY takes (whether or not the walk sends them
there: "walk_routes_to"), per class of layer — 3x3 band
(W <= 94), 3x3 wide or generic (W > 94), 1x1 — through the exact entry and through the split entry, and the split entry's five kernel
groups alone (rtod_conv_dgrad_split_phases): the images' maxima, dz to split planes, the weight pack, the conv, the finish.  Each
helper's time is also given as a multiple of ONE pass over its tensors at 5651.7 GB/s (what tools/ubench_launch measured):
  amax    reads dz                                       split   reads dz, writes the planes (4 B Kc per pixel)
  pack    reads w twice, writes both planes              finish  reads the Cin used columns of the raw rows and y, writes dx
A class whose split time is not below its exact time by more than the rounds' spread is marked "route_exact" with the reason.
Alternating rounds, HIP events around windows of --iters calls, medians."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grad_walk
import torch
from realtimeobjectdetection_amd import cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir

ap = argparse.ArgumentParser()
ap.add_argument("--net", default="yolov3", choices=["yolov3", "tiny"])
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "grad_split_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_grad_split.py measures on the GPU"
LR, GBS = 1e-9, 5651.7

events = lambda fn: grad_walk.events(fn, args.iters)
x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)
if args.net == "yolov3":
    cfg_text, scope, entry, keep = cfgs.yolov3_cfg(args.res, args.res), "backbone", "backbone_gradients", {"keep_head_inputs": 1, "keep_backbone_activations": 1}
else:
    cfg_text, scope, entry, keep = cfgs.yolov3_tiny_cfg(args.res, args.res), "full", "full_gradients", {"keep_head_inputs": 1, "keep_full_activations": 1}
precision = "f16s3" if args.net == "yolov3" else "fp32"           # (YOLOv3-tiny's full scope trains on the exact-fp32 plan)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
trainer = lambda trainable, options: grad_walk.trainer(cfg_text, ir, args.res, precision, trainable, options, LR)
tf, te, ts = trainer("heads", {}), trainer(scope, keep), trainer(scope, keep)
ts.grad_precision = "f16s3"
fns = [lambda: tf._forward_train(x), lambda: te.feed_forward_through_model(x, targets), lambda: ts.feed_forward_through_model(x, targets)]
keys = ["forward", "step_exact", "step_split"]
for f in fns:
    events(f)                                                     # warm-up of every shape the timed windows use

calls, grads = grad_walk.record(te, x, targets, entry)
# a recorded call: (conv_dgrad_async, (w, dz, size, scale, y, slope, stride, hw), {})
taken = [c for c in calls["dgrad"] if grad_walk.stride_of(c) == 1 and T.conv_dgrad_split_takes(c[1][0].size(1), int(c[1][2]))]
klass = lambda c: "1x1" if int(c[1][2]) == 1 else "3x3_band" if c[1][1].size(3) <= 94 else "3x3_wide_or_generic"
classes = {k: [c for c in taken if klass(c) == k] for k in ("3x3_band", "3x3_wide_or_generic", "1x1")}
classes["3x3_all"] = classes["3x3_band"] + classes["3x3_wide_or_generic"]
exact = lambda group: (lambda: [f(*a, **k) for f, a, k in group])
split = lambda group, phases=None: (lambda: [T.conv_dgrad_split_async(a[0], a[1], a[2], a[3], a[4], a[5], phases=phases) for _, a, _ in group])
PHASES = {"amax": 1, "split": 2, "pack": 4, "conv": 8, "finish": 16}
for k, g in classes.items():
    if not g:
        continue
    fns += [exact(g), split(g)]
    keys += [k + ":exact", k + ":split"]
    if k != "3x3_all":
        for name, bit in PHASES.items():
            fns.append(split(g, bit)); keys.append(k + ":phase:" + name)
for f in fns[3:]:
    events(f)
times = [[] for _ in fns]
for r in range(args.rounds):
    for t, f in zip(times, fns):
        t.append(events(f))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
us = {k: statistics.median(t) for k, t in zip(keys, times)}
spread = {k: max(t) - min(t) for k, t in zip(keys, times)}


def traffic(group):
    """Bytes of one pass over each helper's tensors, summed over the group's calls."""
    b = {"amax": 0, "split": 0, "pack": 0, "finish": 0}
    for _, a, _ in group:
        w, dz = a[0], a[1]
        B, cout, H, W = dz.shape
        cin, taps, M = w.size(1), int(a[2]) ** 2, B * H * W
        Kc, Npad = -(-cout // 32) * 32, -(-cin // 128) * 128
        b["amax"] += 4 * dz.numel()
        b["split"] += 4 * dz.numel() + 4 * M * Kc
        b["pack"] += 2 * 4 * w.numel() + 2 * 2 * taps * Kc * Npad
        b["finish"] += 4 * M * cin * (3 if a[4] is not None and a[5] != 1.0 else 2)
    return b


flop = lambda group: sum(2.0 * a[0].numel() * a[1].size(0) * a[1].size(2) * a[1].size(3) for _, a, _ in group)
rows = {}
for k, g in classes.items():
    if not g:
        continue
    e, s = us[k + ":exact"], us[k + ":split"]
    noise = spread[k + ":exact"] + spread[k + ":split"]
    row = {"calls": len(g), "gflop": round(flop(g) / 1e9, 2), "exact_us": round(e, 1), "split_us": round(s, 1), "exact_tflops": round(flop(g) / e / 1e6, 2),
           "split_tflops": round(flop(g) / s / 1e6, 2), "spread_us": round(noise, 1), "faster": bool(e - s > noise)}
    row["walk_routes_to"] = "split" if any(int(a[2]) in T.GRAD_SPLIT_SIZES for _, a, _ in g) else "exact"
    if not row["faster"]:
        row["route_exact"] = "split %.1f us is not below exact %.1f us by more than the rounds' spread %.1f us" % (s, e, noise)
    if k != "3x3_all":
        tr = traffic(g)
        row["phase_us"] = {n: round(us[k + ":phase:" + n], 1) for n in PHASES}
        row["helper_share_of_split"] = round(sum(us[k + ":phase:" + n] for n in PHASES if n != "conv") / s, 3)
        row["helper_x_one_pass"] = {n: round(us[k + ":phase:" + n] / (tr[n] / GBS / 1e3), 2) for n in tr}
        row["conv_tflops"] = round(flop(g) / us[k + ":phase:conv"] / 1e6, 2)
    rows[k] = row
res = {"net": args.net, "res": args.res, "batch": args.batch, "precision": ts.darknet.active_precision, "scope": scope, "boxes_per_image": args.boxes,
       "trainable_convs": len(grads), "loss_exact": float(te.last_components[0].item()), "loss_split": float(ts.last_components[0].item()),
       "status": int(ts.status.item()) | int(te.status.item()),
       "us": {k: round(us[k], 1) for k in keys[:3]}, "spread_us": {k: round(spread[k], 1) for k in keys[:3]},
       "step_exact_over_forward": round(us["step_exact"] / us["forward"], 2), "step_split_over_forward": round(us["step_split"] / us["forward"], 2),
       "step_split_over_step_exact": round(us["step_split"] / us["step_exact"], 3), "entry_takes_calls": len(taken), "walk_split_calls": len([c for c in taken if int(c[1][2]) in T.GRAD_SPLIT_SIZES]), "exact_stride1_calls_left": len([c for c in calls["dgrad"] if grad_walk.stride_of(c) == 1]) - len(taken),
       "classes": rows}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
