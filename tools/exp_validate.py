#!/usr/bin/env python
"""What scoring against ground truth costs on top of detection, in ONE process (synthetic weights, seeded frames):

    python tools/exp_validate.py [--net yolov3] [--res 608] [--batch 8] [--log profiles/experiments/validate_cost.log]

  write_results_async alone                       (the yardstick: README quotes 42 us per batch of 8)
  forward + write_results_async                   against
  forward + write_results_async + score_batch     (alternating rounds, HIP events, medians)
  DarknetValidator.sweep over the reference's 19 NMS thresholds against 19 separate validate_model passes (host clock around
  runs that end in the validator's synchronisation).
Ground truth is made from the network's own detections (jittered, every third dropped), so that the matching loop has work."""
import argparse, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
from realtimeobjectdetection_amd.util import write_results, write_results_async
from realtimeobjectdetection_amd.validate import DarknetValidator

ap = argparse.ArgumentParser()
ap.add_argument("--net", default="yolov3"); ap.add_argument("--res", type=int, default=608); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--conf", type=float, default=0.6); ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--batches", type=int, default=4, help="batches per pass of the sweep comparison")
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "validate_cost.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "exp_validate.py measures on the GPU"

cfg_text = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg}[args.net]()
ir = build_ir(parse_cfg_text(cfg_text), args.res)
with tempfile.TemporaryDirectory() as d:
    m = Darknet(cfgs.write_cfg(os.path.join(d, "t.cfg"), cfg_text), True).eval()
    m.net_info["height"] = args.res
    m.load_weights(synth.write_weights_file(os.path.join(d, "t.weights"), synth.synth_weights(ir)))
x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
with torch.no_grad():
    y = m(x)
    det = write_results(y, 80, args.conf, 0.5)
det = np.zeros((0, 8), np.float32) if isinstance(det, int) else det.cpu().numpy()
classes = tuple(int(c) for c in np.unique(det[:, 7])) or (0,)
rng = np.random.default_rng(1)
targets = []
for b in range(args.batch):
    rows = det[det[:, 0] == b]
    t = np.zeros((len(rows), 85), np.float32)
    box = rows[:, 1:5] + rng.normal(0, 2.0, (len(rows), 4))
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4] = (box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1], 1
    t[np.arange(len(rows)), 5 + rows[:, 7].astype(int)] = 1
    targets.append(torch.from_numpy(t[np.arange(len(rows)) % 3 != 2]).cuda())
v = DarknetValidator(confidence=args.conf, nms_thresh=0.5, resolution=args.res, permitted_classes=classes)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3                 # us per call


def nms_only():
    write_results_async(y, 80, args.conf, 0.5)


def detect():
    with torch.no_grad():
        return write_results_async(m(x), 80, args.conf, 0.5)


def detect_and_score():
    rows, counts = detect()
    v.score_batch(rows, counts, targets)


for f in (nms_only, detect, detect_and_score):
    events(f)                                                     # warm-up of every shape the timed windows use
t_nms, t_det, t_score = [], [], []
for _ in range(args.rounds):
    t_nms.append(events(nms_only)); t_det.append(events(detect)); t_score.append(events(detect_and_score))
batches = [(["f%d_%d" % (k, b) for b in range(args.batch)], x, targets) for k in range(args.batches)]
nmss = [0.05 * i for i in range(19, 0, -1)]
v.sweep(m, batches[:1], nms_thresholds=nmss)                      # warm-up
t0 = time.perf_counter(); swept = v.sweep(m, batches, nms_thresholds=nmss); t_sweep = time.perf_counter() - t0
t0 = time.perf_counter()
separate = []
with open(os.devnull, "w") as null:
    out, sys.stdout = sys.stdout, null
    try:
        for n in nmss:
            w = DarknetValidator(confidence=args.conf, nms_thresh=n, resolution=args.res, permitted_classes=classes)
            w.validate_model(m, batches)
            separate.append(w.total_scores)
    finally:
        sys.stdout = out
t_sep = time.perf_counter() - t0
assert [{k: s[k] for k in ("people_num", "tp", "fp", "fn")} for s in swept] == separate, "sweep differs from separate passes"
med = statistics.median
res = {"net": args.net, "res": args.res, "batch": args.batch, "precision": m.active_precision, "detections": int(len(det)), "targets": int(sum(len(t) for t in targets)),
       "write_results_us": round(med(t_nms), 1), "forward_write_results_us": round(med(t_det), 1), "forward_write_results_score_us": round(med(t_score), 1),
       "scoring_cost_us": round(med(t_score) - med(t_det), 1), "spread_us": [round(max(t) - min(t), 1) for t in (t_nms, t_det, t_score)],
       "sweep19_ms": round(t_sweep * 1e3, 1), "separate19_ms": round(t_sep * 1e3, 1), "sweep_batches": args.batches,
       "sweep_tp_fp_fn": [[s["tp"], s["fp"], s["fn"]] for s in swept[::6]]}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
