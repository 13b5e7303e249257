"""CPU floor of the plain-f16 precision mode (precision 2): the f16 emulation of tests/f16_emulation.py (f16 weights, f16 stored
activations, float32 accumulation on torch CPU) against the fp32 oracle, yolov3 at 416 b2 and 608 b1 and yolov3-tiny at 416 b1 and
608 b2 with the synthetic weights and frames of the golden fixtures.  Per materialised layer: max |emu - ref| / max(1, max |ref|) and rms-relative; on the output:
p99.9 / max of |emu - ref| / max(1, |ref|).  The GPU gates of tests/test_f16_gpu.py are derived from this file.
Usage: python tools/f16_floor.py [profiles/f16_floor.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from realtimeobjectdetection_amd import cfgs, synth  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from f16_emulation import F16Emulation, layer_distance, output_distance  # noqa: E402

CASES = [("yolov3", 416, 2), ("yolov3", 608, 1), ("yolov3-tiny", 416, 1), ("yolov3-tiny", 608, 2)]   # tiny: f16 needs option narrow_cin
SEED = synth.FRAME_SEED   # the frames of tests/golden/fwd_* (synth.synth_frames default)


def floor_case(net, res, B):
    cfg_text = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg}[net]()
    ref = O.RefDarknet(cfg_text, res)
    ref.load_weight_stream(synth.synth_weights(ref.ir))
    x = torch.from_numpy(synth.synth_frames(B, res, seed=SEED))
    emu = F16Emulation(ref)
    with torch.no_grad():
        y_ref, l_ref = ref.forward(x, keep_layers=True)
        y_emu, l_emu = emu.forward(x, keep_layers=True)
    layers = {}
    for i in sorted(l_ref):
        if ref.ir.layers[i].type == "yolo" or i in emu.unstored:
            continue
        layers[str(i)] = layer_distance(l_emu[i].numpy(), l_ref[i].numpy())
    return {"layers": layers, "output": output_distance(y_emu.numpy(), y_ref.numpy()),
            "worst_layer_max_over_absmax": max(v["max_over_absmax"] for v in layers.values()),
            "worst_layer_rms_rel": max(v["rms_rel"] for v in layers.values())}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"what": "plain-f16 emulation (tests/f16_emulation.py) vs the fp32 oracle; synthetic weights, synth_frames default seed",
           "cases": {}}
    for net, res, B in CASES:
        t0 = time.time()
        tag = "%s_%d_b%d" % (net, res, B)
        out["cases"][tag] = floor_case(net, res, B)
        c = out["cases"][tag]
        print(tag, "output", json.dumps(c["output"]), "worst layer max/absmax %.3g rms %.3g" %
              (c["worst_layer_max_over_absmax"], c["worst_layer_rms_rel"]), "(%.0f s)" % (time.time() - t0))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
