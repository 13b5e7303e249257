#!/usr/bin/env python
"""Fixtures of the two checks that used to read the reference checkout at test time (same harness as make_golden.py):

    python tests/golden/make_golden_refcheck.py <reference checkout>

writes tests/golden/ref_cfg_blocks.json (the blocks of the reference's cfg/yolov3.cfg and cfg/yolov3-tiny.cfg as the project's
parse_cfg reads them, only the keys test_generated_cfg_equals_reference_cfg compares) and tests/golden/ref_write_results.npz (the
reference's write_results on the seeded predictions of test_oracle_vs_live_reference_write_results).  Data only: nothing from the
reference is copied."""
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

USED = {"convolutional": ("batch_normalize", "filters", "size", "stride", "pad", "activation"),
        "shortcut": ("from",), "route": ("layers",), "upsample": ("stride",),
        "maxpool": ("size", "stride"), "yolo": ("mask", "anchors", "classes", "num")}
WR_CASES = ((31, 2, 1500, 0.5, 0.4), (32, 1, 4000, 0.7, 0.6), (33, 3, 800, 0.3, 0.5))   # seed, batch, rows, conf, nms


def main(ref):
    import torch
    from realtimeobjectdetection_amd import synth
    from realtimeobjectdetection_amd.cfg import parse_cfg
    blocks = {}
    for net in ("yolov3-tiny", "yolov3"):
        bl = parse_cfg(os.path.join(ref, "cfg", net + ".cfg"))
        blocks[net] = [{"type": bl[0]["type"]}] + [dict([("type", b["type"])] + [(k, b[k]) for k in USED[b["type"]] if k in b])
                                                   for b in bl[1:]]
    json.dump(blocks, open(os.path.join(HERE, "ref_cfg_blocks.json"), "w"), indent=1)

    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref)
    from src.util import write_results
    out = {}
    for seed, B, N, conf, thr in WR_CASES:
        p = synth.synth_predictions(B, N, 80, 416, seed=seed, obj_mu=-2.5)
        out["out_%d" % seed] = write_results(torch.from_numpy(p), 80, conf, thr).numpy()
    np.savez_compressed(os.path.join(HERE, "ref_write_results.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
