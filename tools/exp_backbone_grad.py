#!/usr/bin/env python
"""What training the backbone too (every conv of Darknet.trainable_layers: all of YOLOv3 but layer 0) costs in a training step, in ONE
process (synthetic weights, seeded frames and boxes):

    python tools/exp_backbone_grad.py [--res 416] [--batch 8] [--log profiles/experiments/backbone_grad_cost.log]

for YOLOv3 (f16s3), each path on a model of its own:
  (a) forward under train_mode() on a default plan              the yardstick "one forward"
  (b) the same on a plan with keep_backbone_activations         what holding the shortcut / pointwise / stem2 fusions costs
  (c) feed_forward_through_model, trainable="neck"              forward + heads + every neck conv: the path as it was
  (d) feed_forward_through_model, trainable="backbone"          forward + heads + every trainable conv
and the split of (d)'s walk on (d)'s model, each kernel group alone on the operands of one recorded walk:
  dgrad_s1         rtod_conv_dgrad per conv whose input is in the graph (the 3x3 ones also alone: dgrad3_s1)
  dgrad_s2         rtod_conv_dgrad_s2 per stride-2 conv
  wgrad            rtod_conv_wgrad / rtod_conv_wgrad_s2 per trainable conv (slice kernel + reduce; the stride-2 ones also alone)
  joins            rtod_grad_join per fan-out point and per masked single reader behind a shortcut
  upsample_grad    rtod_upsample2x_grad per upsample
  read_layer       the dense copies the walk takes (inputs for wgrad, outputs for the masks)
  steps            rtod_plan_step_conv_folded per trainable conv (Adam)
Rates are over the USEFUL flops: 2 B Ho Wo k^2 Cout Cin of a conv's data or weight gradient, stride 2 included.  Alternating rounds,
HIP events around windows of --iters calls, medians.  The learning rate is tiny (1e-9): the weights stay where they are over a run,
and no kernel's time depends on them.  The peak of torch's allocator is taken over one backbone step after a reset of its statistics."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grad_walk
import torch
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "backbone_grad_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_backbone_grad.py measures on the GPU"
LR = 1e-9


events = lambda fn: grad_walk.events(fn, args.iters)
trainer = lambda cfg_text, ir, precision, trainable, options: grad_walk.trainer(cfg_text, ir, args.res, precision, trainable, options, LR)
record, stride_of = grad_walk.record, grad_walk.stride_of


x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)

NECK = {"keep_head_inputs": 1, "keep_neck_activations": 1}
BACKBONE = {"keep_head_inputs": 1, "keep_backbone_activations": 1}
net, precision = "yolov3", "f16s3"
cfg_text = cfgs.yolov3_cfg(args.res, args.res)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
ta, tb = trainer(cfg_text, ir, precision, "heads", {}), trainer(cfg_text, ir, precision, "heads", BACKBONE)
tn, tc = trainer(cfg_text, ir, precision, "neck", NECK), trainer(cfg_text, ir, precision, "backbone", BACKBONE)
fns = [lambda: ta._forward_train(x), lambda: tb._forward_train(x), lambda: tn.feed_forward_through_model(x, targets), lambda: tc.feed_forward_through_model(x, targets)]
for f in fns:
    events(f)                                                     # warm-up of every shape the timed windows use (autotune included)
m = tc.darknet
torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
tc.feed_forward_through_model(x, targets)
torch.cuda.synchronize()
peak = int(torch.cuda.max_memory_allocated())
calls, grads = record(tc, x, targets)
replay = lambda group: (lambda: [f(*a, **k) for f, a, k in group])
d1 = [c for c in calls["dgrad"] if stride_of(c) == 1]
d2 = [c for c in calls["dgrad"] if stride_of(c) == 2]
d13 = [c for c in d1 if int(c[1][2]) == 3]
w2 = [c for c in calls["wgrad"] if stride_of(c) == 2]


def steps():
    for layer, dw in grads.items():
        st = tc.optimizer.state[layer]
        m.step_conv_folded(layer, _ffi.OptStep(1, LR, 0.9, 0.999, 1e-8, st["step"] + 1), st["weight"], dw, (st["exp_avg"], st["exp_avg_sq"]))


groups = {"dgrad_s1": d1, "dgrad3_s1": d13, "dgrad_s2": d2, "wgrad": calls["wgrad"], "wgrad_s2": w2, "joins": calls["joins"],
          "upsample_grad": calls["upsample_grad"], "read_layer": calls["read_layer"]}
fns += [replay(g) for g in groups.values()] + [steps]
for f in fns[4:]:
    events(f)
times = [[] for _ in fns]
for r in range(args.rounds):
    for t, f in zip(times, fns):
        t.append(events(f))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
med = [statistics.median(t) for t in times]
spread = [round(max(t) - min(t), 1) for t in times]
keys = ["forward_default", "forward_option", "neck_step", "backbone_step"] + list(groups) + ["steps"]
us = dict(zip(keys, med))
dflop = lambda group: sum(2.0 * a[0].numel() * a[1].size(0) * a[1].size(2) * a[1].size(3) for _, a, _ in group)          # 2 |w| B Ho Wo: dz lives on the conv's output map
wflop = lambda group: sum(2.0 * a[0].size(0) * a[0].size(1) * a[0].size(2) * a[0].size(3) * a[1].size(1) * int(a[2]) ** 2 for _, a, _ in group)
rate = lambda flop, key: round(flop / us[key] / 1e6, 2) if flop else None
s2_rate, s1_rate = rate(dflop(d2), "dgrad_s2"), rate(dflop(d13), "dgrad3_s1")
res = {"net": net, "res": args.res, "batch": args.batch, "precision": m.active_precision, "boxes_per_image": args.boxes,
       "trainable_convs": len(grads), "trainable_weights": int(sum(dw.numel() for dw in grads.values())), "loss": float(tc.last_components[0].item()), "status": int(tc.status.item()),
       "us": {k: round(v, 1) for k, v in us.items()},
       "unfusing_over_forward": round(us["forward_option"] / us["forward_default"], 3),
       "backbone_step_over_forward": round(us["backbone_step"] / us["forward_default"], 2), "backbone_step_over_neck_step": round(us["backbone_step"] / us["neck_step"], 2),
       "calls": {g: len(c) for g, c in groups.items()},
       "gflop": {"dgrad_s1": round(dflop(d1) / 1e9, 2), "dgrad3_s1": round(dflop(d13) / 1e9, 2), "dgrad_s2": round(dflop(d2) / 1e9, 2),
                 "wgrad": round(wflop(calls["wgrad"]) / 1e9, 2), "wgrad_s2": round(wflop(w2) / 1e9, 2)},
       "tflops_useful": {"dgrad3_s1": s1_rate, "dgrad_s2": s2_rate, "wgrad": rate(wflop(calls["wgrad"]), "wgrad"), "wgrad_s2": rate(wflop(w2), "wgrad_s2")},
       "dgrad_s2_below_dgrad3_s1": bool(s2_rate is not None and s1_rate is not None and s2_rate < s1_rate),
       "arena_bytes": {"default": int(ta.darknet._info.arena_bytes), "neck": int(tn.darknet._info.arena_bytes), "backbone": int(m._info.arena_bytes)},
       "torch_peak_bytes_backbone_step": peak,
       "spread_us": dict(zip(keys, spread))}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
