#!/usr/bin/env python
"""What training the whole detection neck (every BatchNorm conv behind the backbone, Darknet.neck_layers) adds to a training step, in
ONE process (synthetic weights, seeded frames and boxes):

    python tools/exp_neck_grad.py [--res 416] [--batch 8] [--log profiles/experiments/neck_grad_cost.log]

for YOLOv3 (f16s3) and YOLOv3-tiny (fp32), each path on a model of its own:
  (a) forward under train_mode()                                the yardstick "one forward" (plan with the neck options)
  (b) feed_forward_through_model, trainable="blocks"            forward + heads + blocks step: the path as it was
  (c) feed_forward_through_model, trainable="neck"              forward + heads + every neck conv
and the split of (c)'s walk on (c)'s model, each kernel group alone on the operands of one recorded walk:
  dgrad            rtod_conv_dgrad per head and neck conv whose input is a neck layer (3x3 ones also alone: dgrad3)
  upsample_grad    rtod_upsample2x_grad per upsample
  read_layer       the dense copies the walk takes (inputs for wgrad, outputs for the masks)
  wgrad            rtod_conv_wgrad per neck conv (slice kernel + reduce)
  steps            rtod_plan_step_conv_folded per neck conv (Adam)
Alternating rounds, HIP events around windows of --iters calls, medians.  The learning rate is tiny (1e-9): the weights stay where
they are over the few thousand steps of a run, and no kernel's time depends on them."""
import argparse, json, os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.train import DarknetTrainer, HeadOptimizer

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "neck_grad_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_neck_grad.py measures on the GPU"
LR = 1e-9


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3                 # us per call


def trainer(cfg_text, ir, precision, trainable, options):
    with tempfile.TemporaryDirectory() as d:
        m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
        m.net_info["height"] = args.res
        m.precision = precision
        m.options = dict(options)
        m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
    t = DarknetTrainer(m, trainable=trainable)
    t.optimizer = HeadOptimizer("adam", lr=LR)
    return t


def record(tc, x, targets):
    """One neck_gradients walk with every kernel call's arguments written down: {group: [(function, args)]}."""
    calls = {"dgrad": [], "upsample_grad": [], "wgrad": [], "read_layer": []}
    names = {"conv_dgrad_async": "dgrad", "upsample2x_grad_async": "upsample_grad", "conv_wgrad_async": "wgrad"}
    saved = {n: getattr(T, n) for n in names}
    read = tc.darknet.read_layer

    def wrap(n):
        def f(*a, **k):
            calls[names[n]].append((saved[n], a, k))
            return saved[n](*a, **k)
        return f
    for n in names:
        setattr(T, n, wrap(n))
    tc.darknet.read_layer = lambda *a, **k: (calls["read_layer"].append((read, a, k)), read(*a, **k))[1]
    try:
        _, _, grads = tc.neck_gradients(x, targets)
    finally:
        for n in names:
            setattr(T, n, saved[n])
        del tc.darknet.read_layer
    return calls, grads


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

BLOCKS = {"keep_head_inputs": 1, "keep_block_inputs": 1}
NECK = {"keep_head_inputs": 1, "keep_neck_activations": 1}
for net, make_cfg, precision in (("yolov3", cfgs.yolov3_cfg, "f16s3"), ("yolov3-tiny", cfgs.yolov3_tiny_cfg, "fp32")):
    cfg_text = make_cfg(args.res, args.res)
    ir = build_ir(parse_cfg_text(cfg_text), args.res)
    ta, tb, tc = trainer(cfg_text, ir, precision, "heads", NECK), trainer(cfg_text, ir, precision, "blocks", BLOCKS), trainer(cfg_text, ir, precision, "neck", NECK)
    plain = trainer(cfg_text, ir, precision, "heads", {})
    plain._forward_train(x)
    fns = [lambda: ta._forward_train(x), lambda: tb.feed_forward_through_model(x, targets), lambda: tc.feed_forward_through_model(x, targets)]
    for f in fns:
        events(f)                                                 # warm-up of every shape the timed windows use (autotune included)
    m = tc.darknet
    calls, grads = record(tc, x, targets)
    replay = lambda group: (lambda: [f(*a, **k) for f, a, k in group])
    three = [c for c in calls["dgrad"] if int(c[1][2]) == 3]

    def steps():
        for layer, dw in grads.items():
            st = tc.optimizer.state[layer]
            m.step_conv_folded(layer, _ffi.OptStep(1, LR, 0.9, 0.999, 1e-8, st["step"] + 1), st["weight"], dw, (st["exp_avg"], st["exp_avg_sq"]))
    groups = ["dgrad", "upsample_grad", "read_layer", "wgrad"]
    fns += [replay(calls[g]) for g in groups] + [replay(three), steps]
    for f in fns[3:]:
        events(f)
    times = [[] for _ in fns]
    for _ in range(args.rounds):
        for t, f in zip(times, fns):
            t.append(events(f))
    med = [statistics.median(t) for t in times]
    spread = [round(max(t) - min(t), 1) for t in times]
    keys = ["forward", "blocks_step", "neck_step"] + groups + ["dgrad3", "steps"]
    dflop = lambda group: sum(2.0 * a[0].numel() * a[1].size(0) * a[1].size(2) * a[1].size(3) for _, a, _ in group)      # 2 * |w| * B * H * W
    wflop = sum(2.0 * a[0].size(0) * a[0].size(2) * a[0].size(3) * a[0].size(1) * a[1].size(1) * int(a[2]) ** 2 for _, a, _ in calls["wgrad"])
    res = {"net": net, "res": args.res, "batch": args.batch, "precision": m.active_precision, "boxes_per_image": args.boxes,
           "neck_convs": sorted(grads), "neck_weights": int(sum(dw.numel() for dw in grads.values())), "loss": float(tc.last_components[0].item()), "status": int(tc.status.item()),
           "forward_us": round(med[0], 1), "blocks_step_us": round(med[1], 1), "neck_step_us": round(med[2], 1), "added_us": round(med[2] - med[1], 1),
           "added_over_forward": round((med[2] - med[1]) / med[0], 3),
           "split_us": {k: round(v, 1) for k, v in zip(keys[3:], med[3:])},
           "calls": {g: len(calls[g]) for g in groups},
           "dgrad_gflop": round(dflop(calls["dgrad"]) / 1e9, 2), "dgrad3_gflop": round(dflop(three) / 1e9, 2), "wgrad_gflop": round(wflop / 1e9, 2),
           "dgrad3_tflops": round(dflop(three) / med[7] / 1e6, 2) if three else None, "wgrad_tflops": round(wflop / med[6] / 1e6, 2),
           "arena_bytes": {"plain": int(plain.darknet._info.arena_bytes), "blocks": int(tb.darknet._info.arena_bytes), "neck": int(m._info.arena_bytes)},
           "spread_us": dict(zip(keys, spread))}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")
    del ta, tb, tc, plain, fns, m, calls, grads
    torch.cuda.empty_cache()
