#!/usr/bin/env python
"""Record the bits of the training path (weight gradients, optimiser steps, host re-packs) on the cases of
tests/test_train_bits_gpu.py: writes tests/golden/train_bits.json.  Needs the GPU.

The record is a before-image: it is taken from the library of the commit named in "recorded_from" and is NOT regenerated when
the code around the kernels changes (the test exists to show that it still gives these bits).
    python tools/dump_train_bits.py COMMIT [FILE]"""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_train_bits_gpu as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.RECORD
digests = {T.wgrad_key(*case): T.wgrad_digest(*case) for case in T.WGRAD_CASES}
with tempfile.TemporaryDirectory() as d:
    for p in T.PRECISIONS:
        digests["step/" + p] = T.step_digest(p, pathlib.Path(d))
for k, v in digests.items():
    print(k, json.dumps(v, sort_keys=True))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_from": commit, "content": "sha256 of the float32 bytes of dW / db, of the packed weight image, and of every master and moment",
               "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
