#!/usr/bin/env python
"""Batch-statistics BatchNorm (module in training mode: what the reference's callers run) for YOLOv3-tiny 416x416 on the exact-fp32
kernels against the split-f16 kernels with the narrow raw-sum instances (options narrow_cin + stem_pool + bn_batch_split +
bn_split_narrow), in ONE process: five plans per batch size —
    fp32           training mode, default options                (today's path: precision "auto" falls back to the exact-fp32 kernels)
    fp32b          the same plan again                           (its distance from `fp32` is the noise floor of this run)
    split          training mode, all options                    (raw-sum narrow / stem instances, statistics, normalise + max-pool in one kernel)
    split_unfused  the same with fuse_bn_pool = 0                (stand-alone normalise and max-pool kernels)
    eval           .eval(), narrow_cin + stem_pool               (the folded split-f16 plan, for scale)
After autotune: forwards timed in interleaved rounds (HIP events around `iters` batches, medians over the rounds), then the
per-launch times of forward_timed (a HIP-event pair around every launch entry, averaged) summed per kernel group.  A BatchNorm
conv's launch entry of the training-mode plans covers its conv, its statistics kernels and its normalise (+ pool) kernel.
    python tools/exp_bn_narrow.py [--batches 1,8,32] [--rounds 5] [--iters 20]"""
import argparse, os, sys, tempfile, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8,32"); ap.add_argument("--res", type=int, default=416)
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
d = tempfile.mkdtemp()
warnings.simplefilter("ignore", RuntimeWarning)              # the training-mode warning
NAMES = ("fp32", "fp32b", "split", "split_unfused", "eval")
SPLIT = {"narrow_cin": 1, "stem_pool": 1, "bn_batch_split": 1, "bn_split_narrow": 1}
PLANS = (("fp32", True, {}), ("fp32b", True, {}), ("split", True, SPLIT), ("split_unfused", True, dict(SPLIT, fuse_bn_pool=0)),
         ("eval", False, {"narrow_cin": 1, "stem_pool": 1}))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def group(li, bn_layers):
    if li.kind in (0, 7):
        if li.layer == 0:
            return "layer 0 (exact fp32 / split stem)"
        if li.layer not in bn_layers:
            return "head convs (no BatchNorm, fused decode)"
        return "BatchNorm convs %dx%d Cin %s" % (li.ksize, li.ksize, "16" if li.cin == 16 else ">= 32")
    return {1: "input pack", 2: "upsample", 4: "maxpool"}.get(li.kind, "other")


res = args.res
text = cfgs.yolov3_tiny_cfg(); w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
for B in (int(s) for s in args.batches.split(",")):
    x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
    models = []
    for name, train, opts in PLANS:
        m = Darknet(cfgs.write_cfg(os.path.join(d, "n.cfg"), text), True)
        if not train:
            m.eval()
        m.net_info["height"] = res; m.overflow_check = "off"; m.update_running_stats = False
        m.options = dict(opts); m.load_weight_stream(w)
        with torch.no_grad():
            m(x); y = m(x).clone()                             # the first forward of a batch size autotunes
        torch.cuda.synchronize()
        models.append((name, m, y))
    by = {n: (m, y) for n, m, y in models}
    desc = by["split"][0].plan_description()
    print("== yolov3-tiny %dx%d batch %d: active precisions %s; bn_raw_bytes %d; fused convs %s" % (
        res, res, B, {n: m.active_precision for n, m, _ in models}, desc.get("bn_raw_bytes", 0),
        [D["index"] for D in desc["layers"] if D["type"] == "convolutional" and D["bn"] and D["fused_into"] >= 0]))
    y0 = by["fp32"][1]
    rel = lambda y: (y - y0).abs() / y0.abs().clamp(min=1.0)
    print("outputs: fp32 == fp32b bitwise: %s; split == split_unfused bitwise: %s; split vs fp32 max |d|/max(1,|ref|) %.3e, p99.9 %.3e" % (
        torch.equal(y0, by["fp32b"][1]), torch.equal(by["split"][1], by["split_unfused"][1]), float(rel(by["split"][1]).max()),
        float(torch.quantile(rel(by["split"][1]).flatten()[::7].float(), 0.999))))
    fwd = {n: [] for n in NAMES}; table = {n: None for n in NAMES}
    with torch.no_grad():
        for r in range(args.rounds):
            for name, m, _y in models:
                for _ in range(3):
                    m(x)
                fwd[name].append(timed(lambda: m(x), args.iters))
                for _ in range(2):
                    _, ms = m.forward_timed(x)
                    table[name] = ms if table[name] is None else table[name] + ms
    med = {k: float(np.median(v)) for k, v in fwd.items()}
    print("%-14s %12s %12s %12s" % ("plan", "forward ms", "(min)", "frames/s"))
    for name in NAMES:
        print("%-14s %12.3f %12.3f %12.1f" % (name, med[name], min(fwd[name]), B * 1e3 / med[name]))
    noise = abs(med["fp32b"] - med["fp32"])
    print("noise floor |fp32b - fp32|: %.3f ms;  split against fp32: %+.3f ms, %.3fx the frames/s (%s the noise floor);  split against split_unfused: %+.3f ms;  "
          "eval split-f16 against split: %.3fx" % (noise, med["split"] - med["fp32"], med["fp32"] / med["split"],
                                                    "faster by more than" if med["fp32"] - med["split"] > noise else "NOT faster by more than",
                                                    med["split"] - med["split_unfused"], med["split"] / med["eval"]))
    bn_layers = {D["index"] for D in desc["layers"] if D["type"] == "convolutional" and D["bn"]}
    t = {n: table[n] / (2 * args.rounds) for n in table}
    groups = {}
    for name, m, _y in models:
        for i, li in enumerate(m.launch_infos()):
            g = groups.setdefault(group(li, bn_layers), {})
            g[name] = g.get(name, 0.0) + float(t[name][i])
    print("-- per kernel group, ms per forward (sum of the per-launch event pairs; each includes the launch gap it ends)")
    print(("%-44s" + " %13s" * 5) % (("group",) + NAMES))
    for gname in sorted(groups):
        print(("%-44s" + " %13.3f" * 5) % ((gname,) + tuple(groups[gname].get(n, 0.0) for n in NAMES)))
    print(("%-44s" + " %13.3f" * 5) % (("sum",) + tuple(sum(g.get(n, 0.0) for g in groups.values()) for n in NAMES)))
    tiles = sorted({li.variant - 100 for li in by["split"][0].launch_infos() if li.kind == 0 and li.variant >= 100 and li.layer in bn_layers})
    print("raw-sum tiles the split plan's autotune chose: %s" % tiles)
    del models, by
    torch.cuda.empty_cache()
