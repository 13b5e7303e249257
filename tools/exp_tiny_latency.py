#!/usr/bin/env python
"""Latency datapoint for SURVEY.md §8(f) row 3: YOLOv3-tiny 416x416 batch 1 (BASELINE configs[0]), forward + write_results, one
stream, HIP-event timed, then the per-launch table of one forward_timed.  Default: precision "auto" without options, which runs
tiny on the exact-fp32 kernels; --narrow-cin sets the plan option narrow_cin, with which f16s3 / f16 (and auto -> f16s3) run it.
--option NAME=VALUE sets any further plan option (repeatable), e.g. --narrow-cin --option stem_pool=1.
python tools/exp_tiny_latency.py [--batch 1] [--res 416] [--precision {auto,fp32,f16s3,f16}] [--narrow-cin] [--option NAME=VALUE ...]"""
import argparse, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.util import write_results_async

ap = argparse.ArgumentParser(); ap.add_argument("--batch", type=int, default=1); ap.add_argument("--res", type=int, default=416)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--precision", choices=["auto", "fp32", "f16s3", "f16"], default="auto")
ap.add_argument("--narrow-cin", action="store_true", help="plan option narrow_cin: the Cin = 16 layer on conv_c16_f16s3 tiles (f16s3 / f16 need it)")
ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE", help="plan option (rtod_plan_set_option), repeatable")
args = ap.parse_args()
cfg_text = cfgs.yolov3_tiny_cfg()
ir = build_ir(parse_cfg_text(cfg_text), args.res)
with tempfile.TemporaryDirectory() as d:
    m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
    m.net_info["height"] = args.res
    m.precision = args.precision
    if args.narrow_cin:
        m.options = {"narrow_cin": 1}
    m.options.update({kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.option})
    m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
print('stage: eager', flush=True)
with torch.no_grad():
    for _ in range(20):
        write_results_async(m(x), 80, 0.6, 0.5, cap=4096)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        write_results_async(m(x), 80, 0.6, 0.5, cap=4096)
    e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / args.iters
print('stage: graph', flush=True)
# the same work replayed as one HIP graph (Darknet.make_graphed): forward + write_results_async
run = m.make_graphed(x, post=lambda y: write_results_async(y, 80, 0.6, 0.5, cap=4096))
for _ in range(20):
    run(x)
torch.cuda.synchronize()
e0.record()
for _ in range(args.iters):
    run(x)
e1.record(); torch.cuda.synchronize()
ms_graph = e0.elapsed_time(e1) / args.iters
print('stage: readback', flush=True)
import time
t0 = time.perf_counter()
for _ in range(args.iters):
    y, (rows, counts) = run(x)
    n = int(counts[0].item())                      # one result on the host per frame: the serving latency
lat = (time.perf_counter() - t0) / args.iters * 1e3
print({"graph_ms_per_batch": round(ms_graph, 4), "graph_frames_per_s": round(args.batch * 1000.0 / ms_graph, 1),
       "graph_latency_with_host_readback_ms": round(lat, 4), "launches": m._info.n_launches})
print({"net": "yolov3-tiny", "res": args.res, "batch": args.batch, "precision": m.active_precision, "options": dict(m.options), "ms_per_batch": round(ms, 4),
       "frames_per_s": round(args.batch * 1000.0 / ms, 1), "gflop_per_frame": round(ir.conv_flops / 1e9, 3)})
# per-launch table of one forward (a HIP-event pair around every launch: each time includes the launch gap it ends)
from realtimeobjectdetection_amd import _ffi
with torch.no_grad():
    m.forward_timed(x)
    _, lms = m.forward_timed(x)
kinds = {0: "conv", 1: "pack", 2: "upsample", 3: "add", 4: "maxpool", 5: "decode", 6: "copy", 7: "stem"}
print("launch layer kind     k s  cin cout  hout wout       us  kernel")
for i, (li, t) in enumerate(zip(m.launch_infos(), lms)):
    name = _ffi.lib().rtod_conv_variant_name(li.variant).decode() if li.kind == 0 else ""
    print("%6d %5d %-8s %d %d %4d %4d %5d %4d %8.1f  %s" % (i, li.layer, kinds.get(li.kind, "?"), li.ksize, li.stride, li.cin, li.cout, li.hout, li.wout, t * 1e3, name))
print("sum of launches: %.1f us" % (float(lms.sum()) * 1e3))
