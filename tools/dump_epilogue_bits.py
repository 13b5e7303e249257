#!/usr/bin/env python
"""Record the bits of every split-f16 conv epilogue on the probes of tests/test_epilogue_bits_gpu.py: writes
tests/golden/epilogue_bits.json.  Needs the GPU.

The record is a before-image: it is taken from the library of the commit named in "recorded_from" and is NOT regenerated when
the kernels change (the test exists to show that they still give these bits).
    python tools/dump_epilogue_bits.py COMMIT [FILE]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_epilogue_bits_gpu as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.RECORD
digests = {}
with tempfile.TemporaryDirectory() as d:
    for n, p in T._pairs():
        digests["%s/%s" % (n, p)] = T.digests(n, p, d)
    for n in T.RAW_PROBES:
        digests["raw/%s" % n] = T.digests(n, "f16s3", d, raw=True)
    digests["hosted/slab_c64"] = T.digests("slab_c64", "f16s3", d, hosted=True)
    digests["stem2/yolov3_96_b3"] = T.stem2_digests(d)
total = 0
for k, v in digests.items():
    total += len(v)
    print("%-28s %3d ids, %d distinct digests: %s" % (k, len(v), len(set(v.values())), " ".join(sorted(v, key=int))))
print("TOTAL %d digests in %d groups" % (total, len(digests)))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_from": commit, "content": "sha256 of the float32 bytes of read_layer(stored_layer), per forced tile id "
               "(stem2: per layer of the fused stem kernel)", "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
