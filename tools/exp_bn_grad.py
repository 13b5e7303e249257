#!/usr/bin/env python
"""What training under batch statistics (a model in .train() with options keep_bn_inputs: BatchNorm backward, gamma and beta trained)
costs beside the frozen-BatchNorm step of the same scope, in ONE process per run (fp32, synthetic weights, seeded frames and boxes):

    python tools/exp_bn_grad.py [--res 416] [--batch 8] [--nets yolov3-tiny,yolov3] [--log profiles/experiments/bn_grad_cost.log]

per net (YOLOv3-tiny: scope "full"; YOLOv3: scope "backbone"), each path on a model of its own:
  (a) forward in .train() under train_mode(), the scope's keep option, no keep_bn_inputs     the batch-statistics forward as it was
  (b) the same with keep_bn_inputs                                                            what keeping the raw conv outputs costs
  (c) feed_forward_through_model on an EVAL twin, same scope                                  the yardstick: the frozen-BatchNorm step
  (d) feed_forward_through_model in batch mode                                                the reference's step
and, alone on the operands of one recorded walk of (d), the rtod_bn_grad launches summed (two per BatchNorm conv), beside the time of
five passes over their tensors — du and z read twice, dz written once — at the --stream-gbps streaming rate (5651.7 GB/s: what
tools/ubench_launch measured on an MI355X).  Alternating rounds, HIP events around windows of --iters calls, medians.  The learning rate is
tiny (1e-9).  Nothing here gates a speed."""
import argparse, json, os, statistics, sys, tempfile, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--nets", default="yolov3-tiny,yolov3")
ap.add_argument("--stream-gbps", type=float, default=5651.7)
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "bn_grad_cost.log"))
args = ap.parse_args()

import grad_walk
import torch
from realtimeobjectdetection_amd import cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet

assert torch.cuda.is_available(), "exp_bn_grad.py measures on the GPU"
warnings.simplefilter("ignore", RuntimeWarning)                    # the training-mode warning of the batch-statistics plans
LR = 1e-9
NETS = {"yolov3-tiny": (cfgs.yolov3_tiny_cfg, "full", "keep_full_activations"), "yolov3": (cfgs.yolov3_cfg, "backbone", "keep_backbone_activations")}
events = lambda fn: grad_walk.events(fn, args.iters)


def trainer(cfg_text, ir, train, trainable, options):
    with tempfile.TemporaryDirectory() as d:
        m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True)
        m = m.train() if train else m.eval()
        m.net_info["height"] = args.res
        m.precision = "fp32"
        m.options = dict(options)
        m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
    t = T.DarknetTrainer(m, trainable=trainable)
    t.optimizer = T.HeadOptimizer("adam", lr=LR)
    return t


def record_bn_grad(t, x, targets):
    calls, saved = [], T.bn_grad_async
    T.bn_grad_async = lambda *a: (calls.append(a), saved(*a))[1]
    try:
        t.batchnorm_gradients(x, targets)
    finally:
        T.bn_grad_async = saved
    return calls, saved


x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
for net in args.nets.split(","):
    make_cfg, scope, keep = NETS[net]
    cfg_text = make_cfg(args.res, args.res)
    ir = build_ir(parse_cfg_text(cfg_text), args.res)
    KEEP = {"keep_head_inputs": 1, keep: 1}
    ta, tb = trainer(cfg_text, ir, True, "heads", KEEP), trainer(cfg_text, ir, True, "heads", dict(KEEP, keep_bn_inputs=1))
    tc, td = trainer(cfg_text, ir, False, scope, KEEP), trainer(cfg_text, ir, True, scope, dict(KEEP, keep_bn_inputs=1))
    fns = [lambda: ta._forward_train(x), lambda: tb._forward_train(x), lambda: tc.feed_forward_through_model(x, targets), lambda: td.feed_forward_through_model(x, targets)]
    for f in fns:
        events(f)                                                  # warm-up of every shape the timed windows use
    calls, bn_grad = record_bn_grad(td, x, targets)
    fns.append(lambda: [bn_grad(*a) for a in calls])
    events(fns[-1])
    times = [[] for _ in fns]
    for r in range(args.rounds):
        for t_, f in zip(times, fns):
            t_.append(events(f))
        print("%s: round %d of %d" % (net, r + 1, args.rounds), file=sys.stderr, flush=True)
    keys = ["forward_train", "forward_train_keep_bn_inputs", "frozen_step_eval_twin", "batch_step", "bn_grad_launches"]
    us = dict(zip(keys, [statistics.median(t_) for t_ in times]))
    nbytes = sum(5 * 4 * a[0].numel() for a in calls)
    floor_us = nbytes / args.stream_gbps / 1e3
    res = {"net": net, "res": args.res, "batch": args.batch, "precision": td.darknet.active_precision, "scope": scope, "boxes_per_image": args.boxes,
           "bn_convs": len(calls), "loss": float(td.last_components[0].item()), "status": int(td.status.item()),
           "us": {k: round(v, 1) for k, v in us.items()},
           "keep_bn_inputs_over_forward": round(us["forward_train_keep_bn_inputs"] / us["forward_train"], 3),
           "batch_step_over_frozen_step": round(us["batch_step"] / us["frozen_step_eval_twin"], 2),
           "bn_grad_five_pass_bytes": nbytes, "stream_gbps": args.stream_gbps, "bn_grad_five_pass_us": round(floor_us, 1),
           "bn_grad_over_five_passes": round(us["bn_grad_launches"] / floor_us, 2),
           "arena_bytes": {"train_keep_scope": int(ta.darknet._info.arena_bytes), "train_keep_bn_inputs": int(tb.darknet._info.arena_bytes),
                           "eval_twin": int(tc.darknet._info.arena_bytes)},
           "spread_us": dict(zip(keys, [round(max(t_) - min(t_), 1) for t_ in times]))}
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")
    del ta, tb, tc, td, fns, calls
    torch.cuda.empty_cache()
