#!/usr/bin/env python
"""f16s3 vs plain f16 (precision 2) on YOLOv3 608 b8, in ONE process (cdna guide 5.4 rule 24), interleaved rounds, medians:
  * single stream: frames/s of back-to-back forwards (HIP events around each block of forwards);
  * two in flight: two plans per precision on two streams, one forward each per step (what bench.py runs);
  * per-group kernel times from per-launch HIP events (forward_timed): 3x3 band (the dominant layers), 1x1, stride-2, stem,
    heads (convs with the fused decode), other.
    python tools/exp_f16_throughput.py out.json [res] [batch] [rounds]"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from realtimeobjectdetection_amd import cfgs, synth  # noqa: E402
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir  # noqa: E402
from realtimeobjectdetection_amd.darknet import Darknet  # noqa: E402

out = sys.argv[1]
res = int(sys.argv[2]) if len(sys.argv) > 2 else 608
B = int(sys.argv[3]) if len(sys.argv) > 3 else 8
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 7
ITERS = 20
PRECS = ("f16s3", "f16")
text = cfgs.yolov3_cfg()
w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
d = tempfile.mkdtemp()


def model(prec):
    m = Darknet(cfgs.write_cfg(os.path.join(d, "m.cfg"), text), True).eval()
    m.net_info["height"] = res
    m.precision = prec
    m.overflow_check = "off"
    m.load_weight_stream(w)
    with torch.no_grad():
        m(x)
        m(x)
    torch.cuda.synchronize()
    return m


models = {p: [model(p), model(p)] for p in PRECS}           # two plans per precision (two in flight)


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
    if "bandd" in name or "band_" in name:
        return "band3x3"
    return "3x3_other"


names = {}
for p in PRECS:
    from realtimeobjectdetection_amd import _ffi
    import ctypes as C
    lib = _ffi.lib()
    m = models[p][0]
    nm = []
    for i in range(m._info.n_launches):
        buf = C.create_string_buffer(256)
        lib.rtod_plan_launch_kernel_name(m._plan, i, buf, 256)
        nm.append(buf.value.decode())
    names[p] = nm
infos = {p: models[p][0].launch_infos() for p in PRECS}
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
single = {p: [] for p in PRECS}
dual = {p: [] for p in PRECS}
groups = {p: [] for p in PRECS}
launch = {p: [] for p in PRECS}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
with torch.no_grad():
    for r in range(ROUNDS):
        for p in (PRECS if r % 2 == 0 else PRECS[::-1]):
            m0, m1 = models[p]
            torch.cuda.synchronize()
            e0.record()
            for _ in range(ITERS):
                m0(x)
            e1.record()
            torch.cuda.synchronize()
            single[p].append(B * ITERS / (e0.elapsed_time(e1) / 1e3))
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
            dual[p].append(2 * B * ITERS / (e0.elapsed_time(e1) / 1e3))
            _, ms = m0.forward_timed(x)
            g = {}
            for li, nm_, t in zip(infos[p], names[p], ms):
                k = group(li, nm_)
                g[k] = g.get(k, 0.0) + float(t)
            groups[p].append(g)
            launch[p].append([float(t) for t in ms])
res_out = {"res": res, "batch": B, "rounds": ROUNDS, "iters": ITERS, "precisions": {}}
for p in PRECS:
    gk = sorted({k for g in groups[p] for k in g})
    res_out["precisions"][p] = {
        "single_stream_fps_median": float(np.median(single[p])), "single_stream_fps": single[p],
        "two_in_flight_fps_median": float(np.median(dual[p])), "two_in_flight_fps": dual[p],
        "group_ms_median": {k: float(np.median([g.get(k, 0.0) for g in groups[p]])) for k in gk},
        "launch_ms_median": [float(v) for v in np.median(np.array(launch[p]), axis=0)],
        "kernels": names[p], "layers": [li.layer for li in infos[p]], "variants": [li.variant for li in infos[p]]}
a, b = res_out["precisions"]["f16s3"], res_out["precisions"]["f16"]
res_out["ratio_single"] = b["single_stream_fps_median"] / a["single_stream_fps_median"]
res_out["ratio_two_in_flight"] = b["two_in_flight_fps_median"] / a["two_in_flight_fps_median"]
res_out["group_ratio_f16_over_f16s3"] = {k: b["group_ms_median"].get(k, 0.0) / v for k, v in a["group_ms_median"].items() if v > 0}
# the dominant band kernel: the f16s3 band launch with the largest median time, and the same launch under f16
i = max((j for j, k in enumerate(a["kernels"]) if "band" in k), key=lambda j: a["launch_ms_median"][j])
res_out["dominant_band_launch"] = {"layer": a["layers"][i], "f16s3_kernel": a["kernels"][i], "f16_kernel": b["kernels"][i],
                              "f16s3_ms": a["launch_ms_median"][i], "f16_ms": b["launch_ms_median"][i],
                              "ratio": b["launch_ms_median"][i] / a["launch_ms_median"][i]}
print(json.dumps({k: v for k, v in res_out.items() if k != "precisions"}, indent=1))
for p in PRECS:
    print(p, "single %.0f fps, two in flight %.0f fps" % (res_out["precisions"][p]["single_stream_fps_median"], res_out["precisions"][p]["two_in_flight_fps_median"]),
          json.dumps({k: round(v, 4) for k, v in res_out["precisions"][p]["group_ms_median"].items()}))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res_out, f, indent=1)
