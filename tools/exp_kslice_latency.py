#!/usr/bin/env python
"""A/B of the plan option k_slices_split in ONE process: three plans per (network, resolution, batch, precision) —
    off     the default plan                                   (the baseline: every kernel it had before the option existed)
    off2    the same plan again                                 (its distance from `off` is the noise floor of this run)
    on      k_slices_split = 1                                  (deep small-grid convs on the K-sliced tiles of conv_ks_f16s3.hip)
after autotune, timed in interleaved rounds: forward + write_results eager and replayed as one HIP graph (HIP events around
`iters` batches, medians over the rounds), then the per-launch times (a HIP-event pair around every launch, averaged) of the
layers the option slices, off against on, with grid, K and the number of slices: the rule in plan_build.cpp (split_slice_chunks)
keeps a class of layers only if it is faster than `off` at batch 1 by more than the printed noise floor.
    python tools/exp_kslice_latency.py [--nets yolov3:608,yolov3:416,tiny:416] [--batches 1,2,8] [--precisions f16s3,f16]
                                       [--rounds 5] [--iters 60]"""
import argparse, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from realtimeobjectdetection_amd import cfgs, synth, _ffi
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.util import write_results_async

ap = argparse.ArgumentParser()
ap.add_argument("--nets", default="yolov3:608,yolov3:416,tiny:416"); ap.add_argument("--batches", default="1,2,8")
ap.add_argument("--precisions", default="f16s3,f16"); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=60)
args = ap.parse_args()
NETS = {"yolov3": (cfgs.yolov3_cfg, {}), "tiny": (cfgs.yolov3_tiny_cfg, {"narrow_cin": 1, "stem_pool": 1})}
d = tempfile.mkdtemp()
post = lambda y: write_results_async(y, 80, 0.6, 0.5, cap=4096)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for spec in args.nets.split(","):
    net, res = spec.split(":"); res = int(res)
    gen, base_opts = NETS[net]
    text = gen(); w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    for precision in args.precisions.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            if net == "tiny" and B == 2:
                continue
            x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
            models = []
            for name, extra in (("off", {}), ("off2", {}), ("on", {"k_slices_split": 1})):
                m = Darknet(cfgs.write_cfg(os.path.join(d, "n.cfg"), text), True).eval()
                m.net_info["height"] = res; m.precision = precision; m.overflow_check = "off"
                m.options = dict(base_opts, **extra); m.load_weight_stream(w)
                with torch.no_grad():
                    m(x); y = m(x).clone()                   # the first forward of a batch size autotunes
                torch.cuda.synchronize()
                models.append((name, m, y, m.make_graphed(x, post=post)))
            y0 = models[0][2]
            print("== %s %dx%d batch %d precision %s" % (net, res, res, B, precision))
            print("outputs: off == off2 bitwise: %s; on vs off max |d|/max(1,|ref|) %.3e" % (
                torch.equal(y0, models[1][2]), float(((models[2][2] - y0).abs() / y0.abs().clamp(min=1.0)).max())))
            eager = {n: [] for n, *_ in models}; graph = {n: [] for n, *_ in models}; table = {n: None for n, *_ in models}
            with torch.no_grad():
                for r in range(args.rounds):
                    for name, m, _y, run in models:
                        for _ in range(3):
                            post(m(x))
                        eager[name].append(timed(lambda: post(m(x)), args.iters))
                        for _ in range(3):
                            run(x)
                        graph[name].append(timed(lambda: run(x), args.iters))
                        for _ in range(2):
                            _, ms = m.forward_timed(x)
                            table[name] = ms if table[name] is None else table[name] + ms
            med = {k: (float(np.median(eager[k])), float(np.median(graph[k]))) for k in eager}
            print("%-6s %12s %12s %12s %12s" % ("plan", "eager ms", "(min)", "graph ms", "(min)"))
            for name, *_ in models:
                print("%-6s %12.4f %12.4f %12.4f %12.4f" % (name, med[name][0], min(eager[name]), med[name][1], min(graph[name])))
            print("noise floor |off2 - off|: eager %.4f ms, graph %.4f ms;  on - off: eager %+.4f ms (%.3fx), graph %+.4f ms (%.3fx)" % (
                abs(med["off2"][0] - med["off"][0]), abs(med["off2"][1] - med["off"][1]), med["on"][0] - med["off"][0], med["off"][0] / med["on"][0],
                med["on"][1] - med["off"][1], med["off"][1] / med["on"][1]))
            t = {n: table[n] / (2 * args.rounds) * 1e3 for n in table}
            on = models[2][1]
            slices = {D["index"]: D["k_slices"] for D in on.plan_description()["layers"] if "k_slices" in D}
            lib = _ffi.lib()
            print("-- sliced layers, per-launch us (each includes the launch gap it ends): off, off2, on; sums %.1f %.1f %.1f" % tuple(
                sum(float(t[n][i]) for i, li in enumerate(on.launch_infos()) if li.kind == 0 and li.layer in slices) for n in ("off", "off2", "on")))
            for i, (lo, ln) in enumerate(zip(models[0][1].launch_infos(), on.launch_infos())):
                if ln.kind != 0 or ln.layer not in slices:
                    continue
                print("L%-3d k%d s%d %4d->%4d @%3dx%-3d K %5d S %2d  %8.1f %8.1f %8.1f  %+7.1f  %s | %s" % (
                    ln.layer, ln.ksize, ln.stride, ln.cin, ln.cout, ln.hout, ln.wout, ln.ksize * ln.ksize * ln.cin, slices[ln.layer],
                    t["off"][i], t["off2"][i], t["on"][i], t["on"][i] - t["off"][i],
                    lib.rtod_conv_variant_name(lo.variant).decode(), lib.rtod_conv_variant_name(ln.variant).decode()))
            del models
            torch.cuda.empty_cache()
