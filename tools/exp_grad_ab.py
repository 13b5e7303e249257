#!/usr/bin/env python
"""A/B of the gradient kernels of several BUILDS of librtod in ONE process, on the kernel groups of tools/exp_backbone_grad.py:

    python tools/exp_grad_ab.py librtod_parent.so librtod.so [more.so ...] [--groups dgrad_s1,neck_step] [--res 416] [--batch 8] [--log FILE]

(names relative to realtimeobjectdetection_amd/; the first library is the yardstick, every other one a candidate; a second copy of
the yardstick among them shows what two loads of the same code differ by).  Both are dlopen'ed privately and
``_ffi._lib`` is switched between them, as tools/exp_ab_libs.py does.  YOLOv3 (f16s3), trainable="backbone": one walk is recorded on
the first library's model and each group of its kernel calls (dgrad_s1, dgrad3_s1, dgrad_s2, wgrad, wgrad_s2: the calls are
functions of tensors alone) is replayed under every library in alternating rounds, the order reversed every round; neck_step and
backbone_step run on a trainer per library.  HIP events around windows of --iters calls, medians over --rounds, spread_us = max - min
over the rounds.  A group PASSES when a candidate's median is not above the yardstick's by more than the yardstick's own spread in
this run.  Before timing, every replayed call's result is compared bit for bit with the yardstick's.
--tiny adds YOLOv3-tiny (fp32), trainable="full": one full_gradients walk is recorded and replayed the same way (tiny_wgrad and tiny_dgrad:
the thin entries of layers 0 and 2 among them) and tiny_full_step runs on a trainer per library."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import grad_walk
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--groups", default="", help="comma-separated subset of the groups (default: all)")
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--boxes", type=int, default=12, help="boxes per image")
ap.add_argument("--tiny", action="store_true", help="also the full walk of YOLOv3-tiny")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "grad_one_loop_ab.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_grad_ab.py measures on the GPU"
here = os.path.dirname(os.path.abspath(_ffi.__file__))
handles = {}
for n in args.libs:
    _ffi.LIB_PATH = os.path.join(here, n); _ffi._lib = None
    handles[n] = _ffi.lib()


def use(n):
    _ffi._lib = handles[n]


x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
targets = grad_walk.boxes(args.batch, args.res, args.boxes)
cfg_text = cfgs.yolov3_cfg(args.res, args.res)
ir = build_ir(parse_cfg_text(cfg_text), args.res)
SCOPES = {"neck_step": ("neck", {"keep_head_inputs": 1, "keep_neck_activations": 1}), "backbone_step": ("backbone", {"keep_head_inputs": 1, "keep_backbone_activations": 1})}
if args.tiny:
    tiny_text = cfgs.yolov3_tiny_cfg(args.res, args.res)
    SCOPES["tiny_full_step"] = ("full", {"keep_head_inputs": 1, "keep_full_activations": 1})
RECORDED = ("backbone_step", "tiny_full_step")                        # the first library's trainers of these record the walks
wanted = args.groups.split(",") if args.groups else None
steps = {k: {} for k in SCOPES}
for n in args.libs:
    use(n)
    for k, (scope, options) in SCOPES.items():
        if wanted is None or k in wanted or (k in RECORDED and n == args.libs[0]):
            tiny = k == "tiny_full_step"                                                  # the weights stay where they are over a run
            t = grad_walk.trainer(tiny_text if tiny else cfg_text, build_ir(parse_cfg_text(tiny_text), args.res) if tiny else ir, args.res, "fp32" if tiny else "f16s3", scope, options, 1e-9)
            steps[k][n] = (lambda t=t: t.feed_forward_through_model(x, targets))
            steps[k][n].trainer = t
            grad_walk.events(steps[k][n], 3)                                 # warm-up of every shape (autotune included)
use(args.libs[0])
calls, _ = grad_walk.record(steps["backbone_step"][args.libs[0]].trainer, x, targets)
dgrads, wgrads, stride_of, events = calls["dgrad"], calls["wgrad"], grad_walk.stride_of, grad_walk.events
d1 = [c for c in dgrads if stride_of(c) == 1]
groups = {"dgrad_s1": d1, "dgrad3_s1": [c for c in d1 if int(c[1][2]) == 3], "dgrad_s2": [c for c in dgrads if stride_of(c) == 2],
          "wgrad": wgrads, "wgrad_s2": [c for c in wgrads if stride_of(c) == 2]}
recorded = dgrads + wgrads
if args.tiny:
    tcalls, _ = grad_walk.record(steps["tiny_full_step"][args.libs[0]].trainer, x, targets, "full_gradients")
    groups.update({"tiny_wgrad": tcalls["wgrad"], "tiny_dgrad": tcalls["dgrad"]})
    recorded = recorded + tcalls["dgrad"] + tcalls["wgrad"]
replay = lambda group: (lambda: [f(*a, **k) for f, a, k in group])

# every library gives the yardstick's bits on every recorded call
results = {}
for n in args.libs:
    use(n)
    results[n] = [f(*a, **k) for f, a, k in recorded]
    torch.cuda.synchronize()
flat = lambda r: [t for v in r for t in (v if isinstance(v, tuple) else (v,)) if t is not None]
differing = {n: sum(not torch.equal(p, q) for p, q in zip(flat(results[args.libs[0]]), flat(results[n]))) for n in args.libs[1:]}
del results

fns = {k: {n: replay(g) for n in args.libs} for k, g in groups.items()}
fns.update(steps)
if wanted:
    fns = {k: fns[k] for k in wanted}
times = {k: {n: [] for n in args.libs} for k in fns}
for k in fns:
    for n in args.libs:
        use(n); events(fns[k][n], 2)
for r in range(args.rounds):
    order = args.libs if r % 2 == 0 else args.libs[::-1]         # neither library always runs first
    for k in fns:
        for n in order:
            use(n)
            times[k][n].append(events(fns[k][n], args.iters))
    print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
a = args.libs[0]
res = {"net": "yolov3 + yolov3-tiny" if args.tiny else "yolov3", "res": args.res, "batch": args.batch, "iters": args.iters, "rounds": args.rounds, "yardstick": a,
       "calls": {k: len(g) for k, g in groups.items()}, "results_differing_in_bits": differing, "groups": {}}
for k in fns:
    ma, sa = statistics.median(times[k][a]), max(times[k][a]) - min(times[k][a])
    res["groups"][k] = {"us_yardstick": round(ma, 1), "spread_us_yardstick": round(sa, 1)}
    for b in args.libs[1:]:
        mb, sb = statistics.median(times[k][b]), max(times[k][b]) - min(times[k][b])
        res["groups"][k][b] = {"us": round(mb, 1), "spread_us": round(sb, 1), "move_us": round(mb - ma, 1), "move_percent": round((mb / ma - 1) * 100, 3),
                               "inside_spread": bool(abs(mb - ma) <= sa), "passes": bool(mb - ma <= sa)}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
