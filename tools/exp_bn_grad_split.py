#!/usr/bin/env python
"""What training under batch statistics costs on the split-f16 kernels (precision "f16s3", options bn_batch_split + keep_bn_inputs)
beside the same step on the exact-fp32 batch plan, in ONE process (synthetic weights, seeded frames and boxes):

    python tools/exp_bn_grad_split.py [--res 416] [--batch 8] [--log profiles/experiments/bn_grad_split_cost.log]

YOLOv3, scope "backbone", each path on a model of its own:
  (a) (b)  forward in .train() under train_mode() on the fp32 batch plan, without and with keep_bn_inputs
  (c) (d)  the same on the split batch plan
  (e) (f)  feed_forward_through_model in batch mode on the fp32 plan and on the split plan
and arena_bytes of the four plans.  Alternating rounds, HIP events around windows of --iters calls, medians.  The learning rate is tiny
(1e-9).  Recorded beside the times, from one batchnorm_gradients call of (e) and (f) on the same weights, frames and boxes: per kind of
parameter the relative difference ||g_split - g_fp32|| / ||g_fp32|| over all trained convs and the largest per-conv one, with the
synthetic head weights and with a tenth of them: the size of the split forward's format error (and of its heads' decode arithmetic)
seen through the backward (both backwards are the same exact-fp32 kernels), beside the distance
of the kept raw sums (read_bn_input) and of the stored activations themselves and the share of leaky masks that differ between the two forwards.  Nothing here gates a speed or
a distance.  The yardstick of the gradient distance is taken in the same run on the exact-fp32 plan alone: its gradients after a
relative perturbation of the input frames by 2^-20."""
import argparse, json, os, statistics, sys, tempfile, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "bn_grad_split_cost.log"))
args = ap.parse_args()

import grad_walk
import torch
from realtimeobjectdetection_amd import cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet

assert torch.cuda.is_available(), "exp_bn_grad_split.py measures on the GPU"
warnings.simplefilter("ignore", RuntimeWarning)                    # the training-mode warning of the batch-statistics plans
LR = 1e-9
SCOPE, KEEP = "backbone", {"keep_head_inputs": 1, "keep_backbone_activations": 1}
events = lambda fn: grad_walk.events(fn, args.iters)


def trainer(cfg_text, ir, precision, trainable, options):
    with tempfile.TemporaryDirectory() as d:
        m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).train()
        m.net_info["height"] = args.res
        m.precision = precision
        m.options = dict(options)
        m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
    t = T.DarknetTrainer(m, trainable=trainable)
    t.optimizer = T.HeadOptimizer("adam", lr=LR)
    return t


x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
cfg_text = cfgs.yolov3_cfg(args.res, args.res)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
SPLIT = dict(KEEP, bn_batch_split=1)
fa, fb = trainer(cfg_text, ir, "fp32", "heads", KEEP), trainer(cfg_text, ir, "fp32", "heads", dict(KEEP, keep_bn_inputs=1))
sa, sb = trainer(cfg_text, ir, "f16s3", "heads", SPLIT), trainer(cfg_text, ir, "f16s3", "heads", dict(SPLIT, keep_bn_inputs=1))
fs, ss = trainer(cfg_text, ir, "fp32", SCOPE, dict(KEEP, keep_bn_inputs=1)), trainer(cfg_text, ir, "f16s3", SCOPE, dict(SPLIT, keep_bn_inputs=1))
# the gradients of both plans on the same state, before any step: once with the synthetic head weights as they are (their sigmoids
# saturate, so p (1 - p) of the loss gradient hangs on the last bits of the decode, which the split plan evaluates with the hardware
# exp2 and the fp32 plan with expf), once with a tenth of them (the tests' tenth_heads: sigmoids that do not saturate)
def distances(other=None, x_other=None):
    """Of ``other``'s gradients (default: the split plan's, on the same frames) from the fp32 plan's."""
    g32 = fs.batchnorm_gradients(x, targets)
    g16 = ss.batchnorm_gradients(x, targets) if other is None else other.batchnorm_gradients(x_other, targets)
    assert sorted(g32[2]) == sorted(g16[2]) and sorted(g32[1]) == sorted(g16[1]) and not ss.darknet.overflowed()
    out = {}
    for name, over, pick in (("head_dW", 1, lambda g, c: g[1][c][0]), ("dW", 2, lambda g, c: g[2][c]), ("dgamma", 2, lambda g, c: g[3][c][0]), ("dbeta", 2, lambda g, c: g[3][c][1])):
        num = {c: float((pick(g16, c).double() - pick(g32, c).double()).norm()) for c in g32[over]}
        den = {c: float(pick(g32, c).double().norm()) for c in g32[over]}
        worst = max(num, key=lambda c: num[c] / den[c])
        if name == "dW":                                           # ... per conv too: how the distance grows with the distance from the heads
            out["dW_per_conv"] = {c: float("%.2g" % (num[c] / den[c])) for c in sorted(num)}
        out[name] = {"all": float("%.3g" % ((sum(v * v for v in num.values()) / sum(v * v for v in den.values())) ** 0.5)), "worst_conv": worst,
                     "worst": float("%.3g" % (num[worst] / den[worst]))}
    return out, g32


def conv_of(m, layer):
    return next(sub for name, sub in m.module_list[layer].named_children() if name.startswith("conv_"))


dist_saturated, _ = distances()
for t in (fs, ss):
    for head, _ in t.darknet.head_layers():
        t.darknet.update_conv(head, conv_of(t.darknet, head).weight.detach() * 0.1, conv_of(t.darknet, head).bias.detach() * 0.1)
    t._head_masters = None                                         # taken again from the model's parameters (no step has run yet)
dist, g32 = distances()
assert fs.darknet.active_precision == "fp32" and ss.darknet.active_precision == "f16s3"
# ... and what the two forwards those gradients came from stored: the relative distance of every trained conv's output, and the share of
# its elements whose sign, the leaky mask of the backward, differs between the plans
flips = total = 0
act, raw = {}, {}
for c in sorted(g32[2]):
    z32, z16 = fs.darknet.read_bn_input(c, args.batch), ss.darknet.read_bn_input(c, args.batch)
    raw[c] = float((z16.double() - z32.double()).norm() / z32.double().norm())
    del z32, z16
    y32, y16 = fs.darknet.read_layer(c, args.batch), ss.darknet.read_layer(c, args.batch)
    act[c] = float((y16.double() - y32.double()).norm() / y32.double().norm())
    flips += int(((y32 > 0) != (y16 > 0)).sum().item())
    total += y32.numel()
    del y32, y16
loss32, loss16 = float(fs.last_components[0].item()), float(ss.last_components[0].item())
# the yardstick of those distances, on the exact-fp32 plan alone: the same gradients after a relative perturbation of the input frames by
# 2^-20 (seeded), which moves the stored activations about as far as the split format does; how far the gradients then move says how
# much the backward of this net at these weights amplifies a forward difference of that size
keep32 = {c: fs.darknet.read_layer(c, args.batch) for c in (1, 35, 60, 80, 92, 104)}
gen = torch.Generator(device="cpu").manual_seed(5)
x_pert = x * (1 + 2.0 ** -20 * (2 * torch.rand(x.shape, generator=gen) - 1).to(x.device))
dist_pert, _ = distances(fs, x_pert)
act_pert = {c: float((fs.darknet.read_layer(c, args.batch).double() - y.double()).norm() / y.double().norm()) for c, y in keep32.items()}
del keep32
fs.batchnorm_gradients(x, targets)
fns = [lambda: fa._forward_train(x), lambda: fb._forward_train(x), lambda: sa._forward_train(x), lambda: sb._forward_train(x),
       lambda: fs.feed_forward_through_model(x, targets), lambda: ss.feed_forward_through_model(x, targets)]
for f in fns:
    events(f)                                                      # warm-up of every shape the timed windows use
assert fa.darknet.active_precision == fb.darknet.active_precision == "fp32" and sa.darknet.active_precision == sb.darknet.active_precision == "f16s3"
times = [[] for _ in fns]
for r in range(args.rounds):
    for t_, f in zip(times, fns):
        t_.append(events(f))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
keys = ["fp32_forward_train", "fp32_forward_train_keep_bn_inputs", "split_forward_train", "split_forward_train_keep_bn_inputs", "fp32_batch_step", "split_batch_step"]
us = dict(zip(keys, [statistics.median(t_) for t_ in times]))
res = {"net": "yolov3", "res": args.res, "batch": args.batch, "scope": SCOPE, "boxes_per_image": args.boxes, "bn_convs": len(g32[2]),
       "loss": {"fp32": loss32, "split": loss16}, "status": int(ss.status.item()), "overflowed": bool(ss.darknet.overflowed()),
       "us": {k: round(v, 1) for k, v in us.items()},
       "split_keep_bn_inputs_over_forward": round(us["split_forward_train_keep_bn_inputs"] / us["split_forward_train"], 3),
       "split_step_over_fp32_step": round(us["split_batch_step"] / us["fp32_batch_step"], 3),
       "arena_bytes": {"fp32": int(fa.darknet._info.arena_bytes), "fp32_keep_bn_inputs": int(fb.darknet._info.arena_bytes),
                       "split": int(sa.darknet._info.arena_bytes), "split_keep_bn_inputs": int(sb.darknet._info.arena_bytes)},
       "gradient_distance_split_vs_fp32": {"tenth_heads": dist, "synthetic_heads_saturated": dist_saturated},
       "stored_activation_distance_split_vs_fp32": {"median": float("%.3g" % statistics.median(act.values())), "worst_conv": max(act, key=act.get), "worst": float("%.3g" % max(act.values()))},
       "bn_input_distance_split_vs_fp32": {"median": float("%.3g" % statistics.median(raw.values())), "worst_conv": max(raw, key=raw.get), "worst": float("%.3g" % max(raw.values()))},
       "fp32_plan_input_perturbed_2^-20": {"gradient_distance": dist_pert, "stored_activation_distance": {c: float("%.3g" % v) for c, v in act_pert.items()},
                                           "split_stored_activation_distance_same_convs": {c: float("%.3g" % act[c]) for c in act_pert}},
       "leaky_mask_flips": {"elements": total, "flipped": flips, "share": float("%.3g" % (flips / total))},
       "spread_us": dict(zip(keys, [round(max(t_) - min(t_), 1) for t_ in times]))}
line = json.dumps(res)
print(line, flush=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
