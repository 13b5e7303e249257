#!/usr/bin/env python
"""Batch-statistics BatchNorm (module in training mode: what the reference's callers run) on the exact-fp32 kernels against
the split-f16 kernels (options = {"bn_batch_split": 1}), YOLOv3, in ONE process: three plans per (resolution, batch) —
    fp32    training mode, default options                      (the path before the option existed: as_run_bn in bench.py)
    fp32b   the same plan again                                 (its distance from `fp32` is the noise floor of this run)
    split   training mode, bn_batch_split = 1, precision auto   (raw-sum conv instances + statistics + bn_apply_split)
and, for scale, `eval`: the folded split-f16 plan of the same network (.eval(), frame-independent).
After autotune: forwards timed in interleaved rounds (HIP events around `iters` batches, medians over the rounds), then the
per-launch times of forward_timed (a HIP-event pair around every launch entry, averaged) summed per kernel group.  A BatchNorm
conv's launch entry of the two training-mode plans covers its conv, its statistics kernels and its normalise kernel; the eval
column shows what the conv alone costs with the BatchNorm folded.
    python tools/exp_bn_split.py [--sizes 608,416] [--batch 8] [--rounds 5] [--iters 20]"""
import argparse, os, sys, tempfile, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="608,416"); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
d = tempfile.mkdtemp()
warnings.simplefilter("ignore", RuntimeWarning)              # the training-mode warning


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
            return "layer 0 (exact fp32 / stem)"
        if li.layer not in bn_layers:
            return "head convs (no BatchNorm, fused decode)"
        return "BatchNorm convs %dx%d stride %d" % (li.ksize, li.ksize, li.stride)
    return {1: "input pack", 2: "upsample", 4: "maxpool"}.get(li.kind, "other")


B = args.batch
for res in (int(s) for s in args.sizes.split(",")):
    text = cfgs.yolov3_cfg(); w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
    models = []
    for name, train, opts in (("fp32", True, {}), ("fp32b", True, {}), ("split", True, {"bn_batch_split": 1}), ("eval", False, {})):
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
    print("== yolov3 %dx%d batch %d: active precisions %s; bn_raw_bytes %d" % (
        res, res, B, {n: m.active_precision for n, m, _ in models}, by["split"][0].plan_description().get("bn_raw_bytes", 0)))
    y0 = by["fp32"][1]
    print("outputs: fp32 == fp32b bitwise: %s; split vs fp32 max |d|/max(1,|ref|) %.3e, p99.9 %.3e" % (
        torch.equal(y0, by["fp32b"][1]), float(((by["split"][1] - y0).abs() / y0.abs().clamp(min=1.0)).max()),
        float(torch.quantile(((by["split"][1] - y0).abs() / y0.abs().clamp(min=1.0)).flatten()[::7].float(), 0.999))))
    fwd = {n: [] for n, *_ in models}; table = {n: None for n, *_ in models}
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
    print("%-6s %12s %12s %12s" % ("plan", "forward ms", "(min)", "frames/s"))
    for name, *_ in models:
        print("%-6s %12.3f %12.3f %12.1f" % (name, med[name], min(fwd[name]), B * 1e3 / med[name]))
    print("noise floor |fp32b - fp32|: %.3f ms;  split against fp32: %+.3f ms, %.3fx the frames/s;  eval split-f16 against split: %.3fx" % (
        abs(med["fp32b"] - med["fp32"]), med["split"] - med["fp32"], med["fp32"] / med["split"], med["split"] / med["eval"]))
    bn_layers = {D["index"] for D in by["split"][0].plan_description()["layers"] if D["type"] == "convolutional" and D["bn"]}
    t = {n: table[n] / (2 * args.rounds) for n in table}
    groups = {}
    for name, m, _y in models:
        for i, li in enumerate(m.launch_infos()):
            g = groups.setdefault(group(li, bn_layers), {})
            g[name] = g.get(name, 0.0) + float(t[name][i])
    print("-- per kernel group, ms per forward (sum of the per-launch event pairs; each includes the launch gap it ends)")
    print("%-44s %9s %9s %9s %9s" % ("group", "fp32", "fp32b", "split", "eval"))
    for gname in sorted(groups):
        print("%-44s %9.3f %9.3f %9.3f %9.3f" % ((gname,) + tuple(groups[gname].get(n, 0.0) for n in ("fp32", "fp32b", "split", "eval"))))
    print("%-44s %9.3f %9.3f %9.3f %9.3f" % (("sum",) + tuple(sum(g.get(n, 0.0) for g in groups.values()) for n in ("fp32", "fp32b", "split", "eval"))))
    tiles = sorted({li.variant - 100 for li in by["split"][0].launch_infos() if li.kind == 0 and li.variant >= 100 and li.layer in bn_layers})
    print("raw-sum tiles the split plan's autotune chose: %s" % tiles)
    del models, by
    torch.cuda.empty_cache()
