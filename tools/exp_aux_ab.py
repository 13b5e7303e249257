#!/usr/bin/env python
"""A/B of the helper kernels (csrc/aux_kernels.hip) of several BUILDS of librtod in ONE process:

    python tools/exp_aux_ab.py librtod_parent.so librtod_parent2.so librtod.so [--rounds 30] [--log FILE]

(names relative to realtimeobjectdetection_amd/; the first library is the yardstick, the second a second copy of the same build — what
two loads of the same code differ by — and every further one a candidate).  All are dlopen'ed privately and ``_ffi._lib`` is switched
between them, as tools/exp_ab_libs.py does.  Per-launch HIP-event times of Darknet.forward_timed, autotune off (every library runs
the same default tiles), in interleaved rounds, the order reversed every round; a round's sample is the mean of two forwards.  Groups:

    tiny_f16s3_helpers   YOLOv3-tiny 416 B 8, f16s3 with narrow_cin + stem_pool, eval: the upsample / add / max-pool / copy launches
    tiny_fp32_helpers    the same net on the exact-fp32 plan
    yolov3_fp32_bn       YOLOv3 416 B 8 in training mode, fp32: the launch entries of the BatchNorm convs (raw conv + statistics + normalise)
    yolov3_split_bn      the same with f16s3 + bn_batch_split

median_us over the rounds; range_us = max - min over the rounds.  spread_us = |median(yardstick) - median(its second copy)|.  A group
PASSES when the candidate's median is not above the yardstick's by more than spread_us.  Before timing, every library's output is
compared bit for bit with the yardstick's."""
import argparse, json, os, statistics, sys, tempfile, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--res", type=int, default=416); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--log", default=os.path.join("profiles", "experiments", "aux_one_body_ab.log"))
args = ap.parse_args()
assert torch.cuda.is_available() and len(args.libs) >= 3, "exp_aux_ab.py measures on the GPU: yardstick, its second copy, candidates"
here = os.path.dirname(os.path.abspath(_ffi.__file__))
handles = {}
for n in args.libs:
    _ffi.LIB_PATH = os.path.join(here, n); _ffi._lib = None
    handles[n] = _ffi.lib()


def use(n):
    _ffi._lib = handles[n]


HELPERS = (2, 3, 4, 6)                                                       # LK_UPSAMPLE, LK_ADD, LK_MAXPOOL, LK_COPY
GROUPS = {"tiny_f16s3_helpers": (cfgs.yolov3_tiny_cfg, "f16s3", {"narrow_cin": 1, "stem_pool": 1}, False),
          "tiny_fp32_helpers": (cfgs.yolov3_tiny_cfg, "fp32", {}, False),
          "yolov3_fp32_bn": (cfgs.yolov3_cfg, "fp32", {}, True),
          "yolov3_split_bn": (cfgs.yolov3_cfg, "f16s3", {"bn_batch_split": 1}, True)}
x = torch.from_numpy(synth.synth_frames(args.batch, args.res)).cuda()
d = tempfile.mkdtemp()
models, picks, differing = {}, {}, {}
warnings.simplefilter("ignore", RuntimeWarning)                              # the training-mode warning
for g, (gen, precision, options, train) in GROUPS.items():
    text = gen(args.res, args.res)
    w = synth.synth_weights(build_ir(parse_cfg_text(text), args.res))
    ref = None
    for n in args.libs:
        use(n)
        m = Darknet(cfgs.write_cfg(os.path.join(d, "m.cfg"), text), True)
        if not train:
            m.eval()
        m.net_info["height"] = args.res; m.precision = precision; m.options = dict(options)
        m.autotune = False; m.update_running_stats = False; m.overflow_check = "off"
        m.load_weight_stream(w)
        with torch.no_grad():
            m(x); y = m(x).clone()
        torch.cuda.synchronize()
        assert m.active_precision == precision, (g, n)
        if ref is None:
            ref = y
            L = m.plan_description()["layers"]
            picks[g] = [k for k, li in enumerate(m.launch_infos()) if (li.kind == 0 and L[li.layer]["bn"] if train else li.kind in HELPERS)]
        else:
            differing[(g, n)] = int((y != ref).sum())
        models[(g, n)] = m
times = {k: [] for k in models}
with torch.no_grad():
    for r in range(args.rounds):
        order = args.libs if r % 2 == 0 else args.libs[::-1]                 # neither library always runs first
        for g in GROUPS:
            for n in order:
                use(n)
                ms = (models[(g, n)].forward_timed(x)[1] + models[(g, n)].forward_timed(x)[1]) / 2
                times[(g, n)].append(float(np.asarray(ms, dtype=np.float64)[picks[g]].sum()) * 1e3)
        print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
a, a2 = args.libs[0], args.libs[1]
res = {"res": args.res, "batch": args.batch, "rounds": args.rounds, "yardstick": a, "second_copy": a2,
       "outputs_differing_in_bits": {"%s/%s" % k: v for k, v in differing.items()}, "groups": {}}
med = lambda k: statistics.median(times[k])
rng = lambda k: max(times[k]) - min(times[k])
for g in GROUPS:
    spread = abs(med((g, a)) - med((g, a2)))
    row = {"launches": len(picks[g]), "median_us_yardstick": round(med((g, a)), 1), "range_us_yardstick": round(rng((g, a)), 1),
           "median_us_second_copy": round(med((g, a2)), 1), "spread_us": round(spread, 1)}
    for b in args.libs[2:]:
        row[b] = {"median_us": round(med((g, b)), 1), "range_us": round(rng((g, b)), 1), "move_us": round(med((g, b)) - med((g, a)), 1),
                  "move_percent": round((med((g, b)) / med((g, a)) - 1) * 100, 3), "passes": bool(med((g, b)) - med((g, a)) <= spread)}
    res["groups"][g] = row
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
with open(args.log, "a") as f:
    f.write(line + "\n")
