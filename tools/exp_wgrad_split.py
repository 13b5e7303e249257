#!/usr/bin/env python
"""What the opt-in split-f16 weight gradients (DarknetTrainer(wgrad_precision="f16s3"): rtod_conv_wgrad_split) change in a training
step, in ONE process (synthetic weights, seeded frames and boxes):

    python tools/exp_wgrad_split.py [--net yolov3|tiny] [--res 416] [--batch 8] [--log profiles/experiments/wgrad_split_cost.log]

YOLOv3 (f16s3, scope backbone; --net tiny: YOLOv3-tiny, fp32, scope full), each path on a model of its own:
  forward                                     forward under train_mode() on a default plan: the yardstick "one forward"
  step:<grad_precision>:<wgrad_precision>     feed_forward_through_model for the four combinations of fp32 / f16s3 (the walk routes the
                                              sizes of train.WGRAD_SPLIT_SIZES, which the line records)
and, on the operands of one recorded exact walk, the stride-1 weight gradients the split ENTRY takes (whether or not the walk sends
them there: "walk_routes_to"), grouped by size — 1x1 and 3x3 — through the exact entry (rtod_conv_wgrad: the yardstick, untouched code)
and through the split entry, and the split entry's four kernel groups alone (rtod_conv_wgrad_split_phases): exponents, split, GEMM,
reduce.  Memory: arena_bytes of the plans, the summed per-shape workspaces of the two entries over the recorded shapes, and the peak
of torch's allocator after the exact step and after the step with split weight gradients.
The rule for train.WGRAD_SPLIT_SIZES: a size stays only if "split_us" is below "exact_us" in the YOLOv3 line of the log.
Alternating rounds, HIP events around windows of --iters calls, medians."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grad_walk
import torch
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir

ap = argparse.ArgumentParser()
ap.add_argument("--net", default="yolov3", choices=["yolov3", "tiny"])
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "wgrad_split_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_wgrad_split.py measures on the GPU"
LR = 1e-9
SHIPPED = tuple(T.WGRAD_SPLIT_SIZES)                                  # what the steps with wgrad_precision="f16s3" route to the split entry

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
COMBOS = [("fp32", "fp32"), ("f16s3", "fp32"), ("fp32", "f16s3"), ("f16s3", "f16s3")]          # (grad_precision, wgrad_precision)
tf = trainer("heads", {})
steps = []
for gp, wp in COMBOS:
    t = trainer(scope, keep)
    t.grad_precision, t.wgrad_precision = gp, wp
    steps.append(t)
fns = [lambda: tf._forward_train(x)] + [(lambda t=t: t.feed_forward_through_model(x, targets)) for t in steps]
keys = ["forward"] + ["step:%s:%s" % c for c in COMBOS]
peaks = {}
for k, f in zip(keys, fns):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    events(f)                                                     # warm-up of every shape the timed windows use
    peaks[k] = int(torch.cuda.max_memory_allocated())

te = steps[0]
calls, grads = grad_walk.record(te, x, targets, entry)
# a recorded call: (conv_wgrad_async, (dz, x, size), {"row_scale": ..., "stride": ...})
stride1 = [c for c in calls["wgrad"] if int(c[2].get("stride", 1)) == 1]
taken = [c for c in stride1 if T.conv_wgrad_split_takes(c[1][1].size(1), int(c[1][2]))]
shape_of = lambda c: (c[1][0].size(0), c[1][0].size(1), c[1][1].size(1), c[1][1].size(2), c[1][1].size(3), int(c[1][2]))
classes = {"1x1": [c for c in taken if int(c[1][2]) == 1], "3x3": [c for c in taken if int(c[1][2]) == 3]}
exact = lambda group: (lambda: [f(*a, **k) for f, a, k in group])
split = lambda group, phases=None: (lambda: [T.conv_wgrad_split_async(a[0], a[1], a[2], k.get("row_scale"), phases=phases) for _, a, k in group])
PHASES = {"exponents": 1, "split": 2, "gemm": 4, "reduce": 8}
n_steps = len(fns)
for k, g in classes.items():
    if not g:
        continue
    fns += [exact(g), split(g)]
    keys += [k + ":exact", k + ":split"]
    for name, bit in PHASES.items():
        fns.append(split(g, bit)); keys.append(k + ":phase:" + name)
for f in fns[n_steps:]:
    events(f)
times = [[] for _ in fns]
for r in range(args.rounds):
    for t, f in zip(times, fns):
        t.append(events(f))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
us = {k: statistics.median(t) for k, t in zip(keys, times)}
spread = {k: max(t) - min(t) for k, t in zip(keys, times)}


def workspace_bytes(entry_name, group):
    """The summed workspace of the entry over the group's DISTINCT shapes (what the per-shape cache holds)."""
    total, n = 0, C.c_size_t()
    for shape in sorted({shape_of(c) for c in group}):
        _ffi.check(getattr(_ffi.lib(), entry_name)(*shape, C.byref(n)))
        total += n.value
    return total


flop = lambda group: sum(2.0 * a[0].size(1) * a[1].size(1) * int(a[2]) ** 2 * a[0].size(0) * a[0].size(2) * a[0].size(3) for _, a, _ in group)
rows = {}
for k, g in classes.items():
    if not g:
        continue
    e, s = us[k + ":exact"], us[k + ":split"]
    noise = spread[k + ":exact"] + spread[k + ":split"]
    rows[k] = {"calls": len(g), "distinct_shapes": len({shape_of(c) for c in g}), "gflop": round(flop(g) / 1e9, 2), "exact_us": round(e, 1), "split_us": round(s, 1),
               "exact_tflops": round(flop(g) / e / 1e6, 2), "split_tflops": round(flop(g) / s / 1e6, 2), "spread_us": round(noise, 1), "split_below_exact": bool(s < e),
               "walk_routes_to": "split" if int(k[0]) in SHIPPED else "exact",
               "phase_us": {n: round(us[k + ":phase:" + n], 1) for n in PHASES}, "gemm_tflops": round(flop(g) / us[k + ":phase:gemm"] / 1e6, 2),
               "workspace_bytes": {"exact": workspace_bytes("rtod_conv_wgrad_workspace", g), "split": workspace_bytes("rtod_conv_wgrad_split_workspace", g)}}
res = {"net": args.net, "res": args.res, "batch": args.batch, "precision": te.darknet.active_precision, "scope": scope, "boxes_per_image": args.boxes,
       "trainable_convs": len(grads), "WGRAD_SPLIT_SIZES": list(SHIPPED),
       "loss": {k: float(t.last_components[0].item()) for k, t in zip(keys[1:], steps)}, "status": max(int(t.status.item()) for t in steps),
       "us": {k: round(us[k], 1) for k in keys[:n_steps]}, "spread_us": {k: round(spread[k], 1) for k in keys[:n_steps]},
       "step_over_exact_step": {k: round(us[k] / us["step:fp32:fp32"], 3) for k in keys[1:n_steps]},
       "stride1_wgrad_calls": len(stride1), "entry_takes_calls": len(taken), "other_wgrad_calls": len(calls["wgrad"]) - len(taken),
       "arena_bytes": {"default": int(tf.darknet._info.arena_bytes), scope: int(te.darknet._info.arena_bytes)}, "allocator_peak_bytes": peaks,
       "classes": rows}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
