#!/usr/bin/env python
"""Square vs rectangular YOLOv3 input in ONE process, interleaved rounds, medians (what a 16:9 camera frame gains when the
network runs 608x352 instead of a letterboxed 608x608):
  * pairs 608x608 / 608x352 (HxW: 608 wide, 352 high) and 416x416 / 416x256, precisions f16s3 and f16, batch 8;
  * single stream: frames/s of back-to-back forwards; two in flight: two plans per shape on two streams (bench.py's shape);
  * full chain per frame batch: 1280x720 uint8 frames (host) -> prep_frames -> forward -> write_results -> rescale_boxes;
  * per-group kernel times (per-launch HIP events, forward_timed): 3x3 band, 1x1, stride-2, stem, heads, other.
    python tools/exp_rect_throughput.py out.json [rounds]
The kernel trace of the rectangular shape alone: tools/exp_rect_throughput.py out.json 1 --only 608x352 under rocprofv3."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import ctypes as C  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from realtimeobjectdetection_amd import _ffi, cfgs, synth  # noqa: E402
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir  # noqa: E402
from realtimeobjectdetection_amd.darknet import Darknet  # noqa: E402
from realtimeobjectdetection_amd.util import prep_frames, rescale_boxes, write_results  # noqa: E402

out = sys.argv[1]
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else 5
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
ITERS = 20
B = 8
PRECS = ("f16s3", "f16")
PAIRS = [((608, 608), (352, 608)), ((416, 416), (256, 416))]       # (height, width): square, rectangle
text = cfgs.yolov3_cfg()
wts = synth.synth_weights(build_ir(parse_cfg_text(text), 416))
d = tempfile.mkdtemp()
shapes = [s for pair in PAIRS for s in pair]
if ONLY:
    hw = tuple(int(v) for v in ONLY.split("x"))
    shapes = [hw]


def model(prec, h, w):
    m = Darknet(cfgs.write_cfg(os.path.join(d, "m.cfg"), text), True).eval()
    m.net_info["height"] = h
    if h != w:
        m.input_width = w
    m.precision = prec
    m.overflow_check = "off"
    m.load_weight_stream(wts)
    return m


def group(li, name):
    if li.kind == 7:
        return "stem"
    if li.kind != 0:
        return "other"
    if li.fused_decode:
        return "heads"
    if li.ksize == 1:
        return "1x1"
    if li.stride == 2:
        return "stride2"
    if "band" in name:
        return "band3x3"
    return "3x3_other"


xs = {(h, w): torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(h * 7 + w)).cuda() for h, w in shapes}
models = {}
for p in PRECS:
    for s in shapes:
        models[(p, s)] = [model(p, *s), model(p, *s)]
        with torch.no_grad():
            for m in models[(p, s)]:
                m(xs[s])
                m(xs[s])
torch.cuda.synchronize()
lib = _ffi.lib()
names, infos = {}, {}
for k, (m, _) in models.items():
    nm = []
    for i in range(m._info.n_launches):
        buf = C.create_string_buffer(256)
        lib.rtod_plan_launch_kernel_name(m._plan, i, buf, 256)
        nm.append(buf.value.decode())
    names[k], infos[k] = nm, m.launch_infos()

frames = np.random.default_rng(0).integers(0, 256, (B, 720, 1280, 3), dtype=np.uint8)        # 16:9 camera frames, host memory
dims = torch.tensor([[1280, 720]] * B, dtype=torch.float32)
single = {k: [] for k in models}
dual = {k: [] for k in models}
chain = {k: [] for k in models}
groups = {k: [] for k in models}
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
keys = list(models)
with torch.no_grad():
    for r in range(ROUNDS):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            (p, s), (m0, m1), x = k, models[k], xs[k[1]]
            torch.cuda.synchronize()
            e0.record()
            for _ in range(ITERS):
                m0(x)
            e1.record()
            torch.cuda.synchronize()
            single[k].append(B * ITERS / (e0.elapsed_time(e1) / 1e3))
            e0.record()
            s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
            for _ in range(ITERS):
                with torch.cuda.stream(s1):
                    m0(x)
                with torch.cuda.stream(s2):
                    m1(x)
            torch.cuda.current_stream().wait_stream(s1); torch.cuda.current_stream().wait_stream(s2)
            e1.record()
            torch.cuda.synchronize()
            dual[k].append(2 * B * ITERS / (e0.elapsed_time(e1) / 1e3))
            t0 = time.perf_counter()
            for _ in range(5):
                xin = prep_frames(frames, (s[1], s[0]), mode="BGR")
                det = write_results(m0(xin), 80, 0.5, 0.4)
                if not isinstance(det, int):
                    rescale_boxes(det, dims, (s[1], s[0]))
            torch.cuda.synchronize()
            chain[k].append(5 * B / (time.perf_counter() - t0))
            _, ms = m0.forward_timed(x)
            g = {}
            for li, nm_, t in zip(infos[k], names[k], ms):
                gk = group(li, nm_)
                g[gk] = g.get(gk, 0.0) + float(t)
            groups[k].append(g)

res = {"batch": B, "rounds": ROUNDS, "iters": ITERS, "shapes": {}}
for k in keys:
    p, (h, w) = k
    gk = sorted({q for g in groups[k] for q in g})
    res["shapes"]["%s %dx%d" % (p, h, w)] = {
        "single_stream_fps_median": float(np.median(single[k])), "two_in_flight_fps_median": float(np.median(dual[k])),
        "chain_fps_median": float(np.median(chain[k])), "group_ms_median": {q: float(np.median([g.get(q, 0.0) for g in groups[k]])) for q in gk},
        "single_stream_fps": single[k], "two_in_flight_fps": dual[k], "chain_fps": chain[k]}
if not ONLY:
    res["ratios_rect_over_square"] = {}
    for p in PRECS:
        for sq, rc in PAIRS:
            a, b = res["shapes"]["%s %dx%d" % ((p,) + sq)], res["shapes"]["%s %dx%d" % ((p,) + rc)]
            res["ratios_rect_over_square"]["%s %dx%d/%dx%d" % ((p,) + rc + sq)] = {
                "pixel_ratio": (sq[0] * sq[1]) / (rc[0] * rc[1]),
                "single": b["single_stream_fps_median"] / a["single_stream_fps_median"],
                "two_in_flight": b["two_in_flight_fps_median"] / a["two_in_flight_fps_median"],
                "chain": b["chain_fps_median"] / a["chain_fps_median"],
                "group_time_ratio": {q: b["group_ms_median"].get(q, 0.0) / v for q, v in a["group_ms_median"].items() if v > 0}}
for k, v in res["shapes"].items():
    print("%-18s single %6.0f fps  two in flight %6.0f fps  chain %6.0f fps  groups %s" % (
        k, v["single_stream_fps_median"], v["two_in_flight_fps_median"], v["chain_fps_median"],
        json.dumps({q: round(t, 3) for q, t in v["group_ms_median"].items()})))
if "ratios_rect_over_square" in res:
    print(json.dumps(res["ratios_rect_over_square"], indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
