#!/usr/bin/env python
"""Record the bits of the training path (weight gradients, optimiser steps, host re-packs) on the cases of
tests/test_train_bits_gpu.py: writes tests/golden/train_bits.json.  Needs the GPU.

The record is a before-image: it is taken from the library of the commit named in "recorded_from" and is NOT regenerated when
the code around the kernels changes (the test exists to show that it still gives these bits).
    python tools/dump_train_bits.py COMMIT [FILE]
    python tools/dump_train_bits.py --grad COMMIT [FILE]    only tests/golden/grad_bits.json: the data gradients and the stride-2 weight
                                                            gradient on that file's GRAD_CASES; train_bits.json is left alone
    python tools/dump_train_bits.py --thin COMMIT [FILE]    only tests/golden/thin_bits.json: the thin-conv gradients on that file's
                                                            THIN_CASES and one full_gradients walk"""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_train_bits_gpu as T  # noqa: E402

args = [a for a in sys.argv[1:] if a not in ("--grad", "--thin")]
grad, thin = "--grad" in sys.argv[1:], "--thin" in sys.argv[1:]
commit = args[0]
out = args[1] if len(args) > 1 else T.GRAD_RECORD if grad else T.THIN_RECORD if thin else T.RECORD
if grad:
    digests = {T.grad_key(*case): T.grad_digest(*case) for case in T.GRAD_CASES}
    content = "sha256 of the float32 bytes of dx, or of dW / db"
elif thin:
    digests = {T.thin_key(*case): T.thin_digest(*case) for case in T.THIN_CASES}
    content = "sha256 of the float32 bytes of dW or dx, and of every trained conv's dW of one full_gradients walk"
    with tempfile.TemporaryDirectory() as d:
        digests[T.THIN_WALK] = T.walk_digest(pathlib.Path(d))
else:
    digests = {T.wgrad_key(*case): T.wgrad_digest(*case) for case in T.WGRAD_CASES}
    content = "sha256 of the float32 bytes of dW / db, of the packed weight image, and of every master and moment"
    with tempfile.TemporaryDirectory() as d:
        for p in T.PRECISIONS:
            digests["step/" + p] = T.step_digest(p, pathlib.Path(d))
for k, v in digests.items():
    print(k, json.dumps(v, sort_keys=True))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_from": commit, "content": content, "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
