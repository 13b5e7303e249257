#!/usr/bin/env python
"""What training the detection blocks (the BatchNorm conv in front of each head conv) adds to a head training step, in ONE process
(synthetic weights, seeded frames and boxes):

    python tools/exp_block_grad.py [--res 416] [--batch 8] [--log profiles/experiments/block_grad_cost.log]

for YOLOv3 (f16s3) and YOLOv3-tiny (fp32), each path on a model of its own:
  (a) forward under train_mode()                                the yardstick "one forward" (plan with both keep options)
  (b) feed_forward_through_model, trainable="heads"             forward + head training step: the path as it was (keep_head_inputs only)
  (c) feed_forward_through_model, trainable="blocks"            (b) + dgrad, read_layer of the block inputs, wgrad, folded steps
and the split of the addition on (c)'s model, each kernel group alone on operands of the last step:
  dgrad            rtod_conv1x1_dgrad per block
  read_layer       the copies of the block inputs (NHWC view -> dense NCHW float32)
  wgrad            rtod_conv_wgrad per block (slice kernel + reduce)
  steps            rtod_plan_step_conv_folded per block (Adam)
Alternating rounds, HIP events around windows of --iters calls, medians.  The learning rate is tiny (1e-9): the weights stay where
they are over the few thousand steps of a run, and no kernel's time depends on them."""
import argparse, json, os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.train import DarknetTrainer, HeadOptimizer, conv1x1_dgrad_async, conv_wgrad_async

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "block_grad_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_block_grad.py measures on the GPU"
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

BOTH = {"keep_head_inputs": 1, "keep_block_inputs": 1}
for net, make_cfg, precision in (("yolov3", cfgs.yolov3_cfg, "f16s3"), ("yolov3-tiny", cfgs.yolov3_tiny_cfg, "fp32")):
    cfg_text = make_cfg(args.res, args.res)
    ir = build_ir(parse_cfg_text(cfg_text), args.res)
    ta, tb, tc = trainer(cfg_text, ir, precision, "heads", BOTH), trainer(cfg_text, ir, precision, "heads", {"keep_head_inputs": 1}), trainer(cfg_text, ir, precision, "blocks", BOTH)
    fns = [lambda: ta._forward_train(x), lambda: tb.feed_forward_through_model(x, targets), lambda: tc.feed_forward_through_model(x, targets)]
    for f in fns:
        events(f)                                                 # warm-up of every shape the timed windows use (autotune included)
    # the split: operands of (c)'s last step
    m = tc.darknet
    blocks = [(h, b, i) for h, b, i in m.head_blocks() if b >= 0]
    B = args.batch
    dzs = [torch.randn((B, 255) + tuple(m.read_layer(h - 1, B).shape[2:]), device=x.device) * 1e-3 for h, _, _ in blocks]
    ys = [m.read_layer(h - 1, B) for h, _, _ in blocks]
    xs = [m.read_layer(i, B) for _, _, i in blocks]
    sizes = [m.module_list[b][0].kernel_size[0] for _, b, _ in blocks]
    scales = [m.conv_scale(b)[0] for _, b, _ in blocks]
    dys = [conv1x1_dgrad_async(tc._head_masters[h][0], dz, y, 0.1) for (h, _, _), dz, y in zip(blocks, dzs, ys)]
    dws = [conv_wgrad_async(dy, xi, s, row_scale=sc)[0] for dy, xi, s, sc in zip(dys, xs, sizes, scales)]

    def steps():
        for (_, b, _), dw in zip(blocks, dws):
            st = tc.optimizer.state[b]
            m.step_conv_folded(b, _ffi.OptStep(1, LR, 0.9, 0.999, 1e-8, st["step"] + 1), st["weight"], dw, (st["exp_avg"], st["exp_avg_sq"]))
    fns += [lambda: [conv1x1_dgrad_async(tc._head_masters[h][0], dz, y, 0.1) for (h, _, _), dz, y in zip(blocks, dzs, ys)],
            lambda: [m.read_layer(i, B) for _, _, i in blocks],
            lambda: [conv_wgrad_async(dy, xi, s, row_scale=sc) for dy, xi, s, sc in zip(dys, xs, sizes, scales)],
            steps]
    for f in fns[3:]:
        events(f)
    times = [[] for _ in fns]
    for _ in range(args.rounds):
        for t, f in zip(times, fns):
            t.append(events(f))
    med = [statistics.median(t) for t in times]
    spread = [round(max(t) - min(t), 1) for t in times]
    wgrad_flop = sum(2.0 * B * dy.shape[2] * dy.shape[3] * dw.numel() for dy, dw in zip(dys, dws))
    dgrad_flop = sum(2.0 * dz.shape[1] * dy.numel() for dz, dy in zip(dzs, dys))
    res = {"net": net, "res": args.res, "batch": B, "precision": m.active_precision, "boxes_per_image": args.boxes,
           "blocks": [b for _, b, _ in blocks], "block_weights": int(sum(dw.numel() for dw in dws)), "loss": float(tc.last_components[0].item()), "status": int(tc.status.item()),
           "forward_us": round(med[0], 1), "heads_step_us": round(med[1], 1), "blocks_step_us": round(med[2], 1), "added_us": round(med[2] - med[1], 1),
           "added_over_forward": round((med[2] - med[1]) / med[0], 3),
           "split_us": {"dgrad": round(med[3], 1), "read_layer": round(med[4], 1), "wgrad": round(med[5], 1), "steps": round(med[6], 1)},
           "wgrad_gflop": round(wgrad_flop / 1e9, 2), "dgrad_gflop": round(dgrad_flop / 1e9, 2), "wgrad_tflops": round(wgrad_flop / med[5] / 1e6, 2),
           "arena_bytes": [int(tb.darknet._info.arena_bytes), int(m._info.arena_bytes)],
           "spread_us": {"forward": spread[0], "heads_step": spread[1], "blocks_step": spread[2], "dgrad": spread[3], "read_layer": spread[4], "wgrad": spread[5], "steps": spread[6]}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")
    del ta, tb, tc, fns, m
    torch.cuda.empty_cache()
