#!/usr/bin/env python
"""Record the bits of the helper kernels (csrc/aux_kernels.hip) on the cases of tests/test_aux_bits_gpu.py: writes
tests/golden/aux_bits.json.  Needs the GPU.

The record is a before-image: it is taken from the library of the commit named in "recorded_from" and is NOT regenerated when
the kernels change (the test exists to show that they still give these bits).
    python tools/dump_aux_bits.py COMMIT [FILE]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_aux_bits_gpu as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.RECORD
digests = {}
for name in sorted(T.CASES):
    with tempfile.TemporaryDirectory() as d:
        got = T.run_case(name, d)
    if got is None:
        print("%-36s refused by prepare: not recorded" % name)
        continue
    digests[name] = got
    print("%-36s %2d keys: %s" % (name, len(got), " ".join(sorted(got))), flush=True)
print("TOTAL %d keys in %d cases" % (sum(len(v) for v in digests.values()), len(digests)))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_from": commit, "content": "per case of tests/test_aux_bits_gpu.py: sha256 of the float32 bytes of read_layer(layer), sha256 of the "
               "float64 (mean, variance) of rtod_plan_bn_batch_stats per BatchNorm layer, the range flag", "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
