#!/usr/bin/env python
"""Record the bits of the LDS-staged split-f16 convs (generic, 16-channel, K-sliced) on the probes of
tests/test_staged_bits_gpu.py: writes tests/golden/staged_conv_bits.json.  Needs the GPU.

The record is a before-image: it is taken from the library of the commit named in "recorded_from" and is NOT regenerated when
the kernels change (the test exists to show that they still give these bits).
    python tools/dump_staged_bits.py COMMIT [FILE]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_staged_bits_gpu as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.RECORD
with tempfile.TemporaryDirectory() as d:
    digests = {"%s/%s" % (n, p): T.digest(n, p, d) for n in T.PROBES for p in T.PRECISIONS}
for k, v in digests.items():
    print(k, v["tile"], v["sha256"])
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_from": commit, "content": "sha256 of the float32 bytes of read_layer(stored_layer), heuristic tile",
               "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
