#!/usr/bin/env python
"""A/B of what the PYTHON package spends per call, several copies of the package in ONE process over one librtod.so:

    python tools/exp_python_call_path_ab.py PARENT_DIR . [PARENT_COPY_DIR ...] [--groups tiny_forward,backbone_step] [--log FILE]

Every argument is a directory that holds a ``realtimeobjectdetection_amd`` package (sources alone will do: every copy loads the
library of this tree).  The first is the yardstick, every other one a candidate; a second copy of the yardstick among them shows
what two loads of the same code differ by.  The copies are imported under names of their own and run in alternating rounds, the
order reversed every round, in the manner of tools/exp_grad_ab.py.

  tiny_forward    ``Darknet.forward`` of YOLOv3-tiny 416x416 batch 1, f16s3 (option narrow_cin): windows of --iters calls with no
                  synchronisation inside, the most host-bound path.  host_us: wall clock until the last call returned;
                  us: HIP events around the window
  backbone_step   one ``feed_forward_through_model`` of YOLOv3 416x416 batch 8, trainable="backbone", to completion (HIP events)

Medians over --rounds, spread_us = max - min over the rounds.  A group PASSES when a candidate's median is not above the
yardstick's by more than the yardstick's own spread in this run."""
import argparse, importlib.util, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("RTOD_LIB", os.path.join(ROOT, "realtimeobjectdetection_amd", "librtod.so"))   # (an absolute path wins over the copy's own directory)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("packages", nargs="+")
ap.add_argument("--groups", default="tiny_forward,backbone_step")
ap.add_argument("--iters", type=int, default=200, help="calls per window of tiny_forward (backbone_step: a tenth)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "python_call_path_ab.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_python_call_path_ab.py measures on the GPU"


def load(index, directory):
    """The package of ``directory`` under a name of its own; its submodules import each other relatively, so they stay apart."""
    name = "rtod_copy_%d" % index
    pkg = os.path.join(os.path.abspath(directory), "realtimeobjectdetection_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    sys.modules[name] = module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return {m: importlib.import_module(name + "." + m) for m in ("cfgs", "synth", "cfg", "darknet", "train", "_ffi")}


labels = ["%d:%s" % (i, p) for i, p in enumerate(args.packages)]
copies = {l: load(i, p) for i, (l, p) in enumerate(zip(labels, args.packages))}


def model(P, cfg_text, res, precision, options):
    ir = P["cfg"].build_ir(P["cfg"].parse_cfg_text(cfg_text), res)
    with tempfile.TemporaryDirectory() as d:
        m = P["darknet"].Darknet(P["cfgs"].write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
        m.net_info["height"] = res
        m.precision, m.options = precision, dict(options)
        m.load_weights(P["synth"].write_weights_file(os.path.join(d, "t.weights"), P["synth"].synth_weights(ir)))
    return m


def boxes(batch, res, per_image=12):
    rng = np.random.default_rng(1)
    out = []
    for _ in range(batch):
        t = np.zeros((per_image, 85), np.float32)
        t[:, 0:2] = rng.uniform(1, res - 1, (per_image, 2))
        t[:, 2:4] = rng.uniform(12, res / 2, (per_image, 2))
        t[:, 4] = 1
        t[np.arange(per_image), 5 + rng.choice([0, 0, 0, 0, 16], per_image)] = 1
        out.append(torch.from_numpy(t).cuda())
    return out


def window(fn, iters):
    """``(us per call by HIP events, host us per call until the last call returned)`` of ``iters`` calls without a synchronisation."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, host / iters * 1e6


wanted = args.groups.split(",")
fns, iters = {}, {}
if "tiny_forward" in wanted:
    fns["tiny_forward"], iters["tiny_forward"] = {}, args.iters
    for l, P in copies.items():
        m = model(P, P["cfgs"].yolov3_tiny_cfg(416, 416), 416, "f16s3", {"narrow_cin": 1})
        m.overflow_check = "off"
        x1 = torch.from_numpy(P["synth"].synth_frames(1, 416)).cuda()
        fns["tiny_forward"][l] = (lambda m=m, x1=x1: m(x1))
if "backbone_step" in wanted:
    fns["backbone_step"], iters["backbone_step"] = {}, max(args.iters // 10, 1)
    for l, P in copies.items():
        m = model(P, P["cfgs"].yolov3_cfg(416, 416), 416, "f16s3", {"keep_head_inputs": 1, "keep_backbone_activations": 1})
        t = P["train"].DarknetTrainer(m, trainable="backbone")
        t.optimizer = P["train"].HeadOptimizer("adam", lr=1e-9)                # (the weights stay where they are over a run)
        x8, targets = torch.from_numpy(P["synth"].synth_frames(8, 416)).cuda(), boxes(8, 416)
        fns["backbone_step"][l] = (lambda t=t, x8=x8, targets=targets: t.feed_forward_through_model(x8, targets))
with torch.no_grad():
    for k in fns:
        for l in labels:
            window(fns[k][l], 3)                                                # warm-up of every shape (autotune included)
    times = {k: {l: [] for l in labels} for k in fns}
    for r in range(args.rounds):
        for k in fns:
            for l in (labels if r % 2 == 0 else labels[::-1]):                  # no copy always runs first
                times[k][l].append(window(fns[k][l], iters[k]))
        print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)

a = labels[0]
res = {"packages": labels, "yardstick": a, "rounds": args.rounds, "iters": iters, "groups": {}}
for k in fns:
    res["groups"][k] = {}
    for j, what in enumerate(("us", "host_us")):
        col = lambda l: [t[j] for t in times[k][l]]
        ma, sa = statistics.median(col(a)), max(col(a)) - min(col(a))
        g = res["groups"][k][what] = {"yardstick": round(ma, 1), "spread_yardstick": round(sa, 1)}
        for b in labels[1:]:
            mb = statistics.median(col(b))
            g[b] = {"median": round(mb, 1), "spread": round(max(col(b)) - min(col(b)), 1), "move": round(mb - ma, 1),
                    "move_percent": round((mb / ma - 1) * 100, 2), "passes": bool(mb - ma <= sa)}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
