#!/usr/bin/env python
"""A/B of the plan option stem_pool on YOLOv3-tiny in ONE process: three plans per (precision, batch) —
    narrow      options narrow_cin                                (pack + exact-fp32 layer 0 + max-pool: the baseline)
    stem_pool   + stem_pool                                       (16-filter split-f16 stem with the max-pool fused)
    unfused     + stem_pool, fuse_stem_pool = 0                   (the same stem stand-alone + max-pool kernel)
timed in interleaved rounds: forward + write_results eager and replayed as one HIP graph (HIP events around `iters` batches),
then the per-launch table (a HIP-event pair around every launch, averaged over the rounds).
    python tools/exp_stem_pool.py [--res 416] [--batches 1,8,32] [--precisions f16s3,f16] [--rounds 6] [--iters 50]"""
import argparse, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from realtimeobjectdetection_amd import cfgs, synth, _ffi
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.util import write_results_async

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batches", default="1,8,32"); ap.add_argument("--precisions", default="f16s3,f16")
ap.add_argument("--rounds", type=int, default=6); ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
PLANS = [("narrow", {"narrow_cin": 1}), ("stem_pool", {"narrow_cin": 1, "stem_pool": 1}), ("unfused", {"narrow_cin": 1, "stem_pool": 1, "fuse_stem_pool": 0})]
KINDS = {0: "conv", 1: "pack", 2: "upsample", 3: "add", 4: "maxpool", 5: "decode", 6: "copy", 7: "stem"}
text = cfgs.yolov3_tiny_cfg(); ir = build_ir(parse_cfg_text(text), args.res)
w = synth.synth_weights(ir)
d = tempfile.mkdtemp()
post = lambda y: write_results_async(y, 80, 0.6, 0.5, cap=4096)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for precision in args.precisions.split(","):
    for B in (int(b) for b in args.batches.split(",")):
        x = torch.from_numpy(synth.synth_frames(B, args.res)).cuda()
        models = []
        for name, opts in PLANS:
            m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), text), True).eval()
            m.net_info["height"] = args.res; m.precision = precision; m.overflow_check = "off"
            m.options = dict(opts); m.load_weight_stream(w)
            with torch.no_grad():
                m(x); y = m(x).clone()
            torch.cuda.synchronize()
            run = m.make_graphed(x, post=post)
            models.append((name, m, y, run))
        y0 = models[0][2]
        print("== yolov3-tiny %dx%d batch %d precision %s" % (args.res, args.res, B, precision))
        print("outputs: stem_pool == unfused bitwise: %s; stem_pool vs narrow max |d|/max(1,|ref|) %.3e" % (
            torch.equal(models[1][2], models[2][2]), float(((models[1][2] - y0).abs() / y0.abs().clamp(min=1.0)).max())))
        eager = {n: [] for n, *_ in models}; graph = {n: [] for n, *_ in models}; table = {n: None for n, *_ in models}
        with torch.no_grad():
            for r in range(args.rounds):
                for name, m, _y, run in models:
                    for _ in range(5):
                        post(m(x))
                    eager[name].append(timed(lambda: post(m(x)), args.iters))
                    for _ in range(5):
                        run(x)
                    graph[name].append(timed(lambda: run(x), args.iters))
                    for _ in range(3):
                        _, ms = m.forward_timed(x)
                        table[name] = ms if table[name] is None else table[name] + ms
        print("%-10s %9s %12s %12s %12s %12s %12s" % ("plan", "launches", "eager ms", "(min)", "graph ms", "(min)", "graph fps"))
        for name, m, _y, run in models:
            e, g = np.array(eager[name]), np.array(graph[name])
            print("%-10s %9d %12.4f %12.4f %12.4f %12.4f %12.1f" % (name, m._info.n_launches, np.median(e), e.min(), np.median(g), g.min(), B * 1000.0 / np.median(g)))
        for name, m, _y, run in models:
            t = table[name] / (3 * args.rounds) * 1e3
            print("-- %s: per-launch us (each includes the launch gap it ends); sum %.1f" % (name, float(t.sum())))
            for i, (li, v) in enumerate(zip(m.launch_infos(), t)):
                nm = _ffi.lib().rtod_conv_variant_name(li.variant).decode() if li.kind == 0 else ""
                gbs = ("%7.0f GB/s" % (li.bytes_per_frame * B / (v * 1e-6) / 1e9)) if v > 0 and li.bytes_per_frame and li.kind != 0 else ""
                print("%4d L%-3d %-8s k%d s%d %4d->%4d @%3dx%-3d %8.1f %s %s" % (i, li.layer, KINDS.get(li.kind, "?"), li.ksize, li.stride, li.cin, li.cout, li.hout, li.wout, v, gbs, nm))
        del models
        torch.cuda.empty_cache()
