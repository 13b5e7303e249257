#!/usr/bin/env python
"""Fixture that pins the device Adam step of the detection heads to torch's own optimiser:

    python tests/golden/make_golden_adam.py

writes tests/golden/adam_step.npz.  torch on the CPU and numpy only; nothing of the reference is read (its trainer builds
``optim.Adam(self.darknet.parameters(), lr=1e-2)``, and that constructor call is all this file restates).

Cases: one 255 x 512 step at each of t = 1, 2, 10, 1000 (tests/head_opt_cases.py: ``adam_inputs``).  The inputs are drawn from a
recorded RandomState seed and not stored: the tests regenerate them and check the recorded checksum.  Per case:
  * ``w64`` / ``m64`` / ``v64``: float64 ``torch.optim.Adam`` from the float32 state, rows ``STORED_ROWS`` (the whole arrays of four
    cases are 12 MiB; the tests recompute the rest with ``adam_ref64`` and hold that to these rows);
  * ``floor_w`` / ``floor_m`` / ``floor_v``: (max, rms) of float32 ``torch.optim.Adam`` on the CPU against that float64 result, in units
    of D_w, D_m, D_v (head_opt_cases), over the whole arrays.  Elements with D = 0 were exact (asserted here)."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))


def main():
    import torch
    import head_opt_cases as A
    out = {"steps": np.asarray(A.STEPS, np.int64), "stored_rows": np.asarray(A.STORED_ROWS, np.int64), "torch_version": np.asarray(torch.__version__)}
    rows = list(A.STORED_ROWS)
    for idx, t in enumerate(A.STEPS):
        k = "c%d_" % idx
        seed = A.SEED0 + idx
        inp = A.adam_inputs(seed, t)
        r64 = A.torch_adam(*inp, t, torch.float64)
        r32 = A.torch_adam(*inp, t, torch.float32)
        d = A.scales(inp[0], inp[1], inp[2], r64)
        mine = A.adam_ref64(*inp, t)
        for a, b, dd in zip(mine, r64, d):                             # the numpy restatement is torch's float64 step
            assert (np.abs(a - b) <= 1e-12 * dd / A.U).all(), t
        out[k + "seed"] = np.int64(seed)
        out[k + "crc"] = np.int64(A.inputs_crc(inp))
        line = ["t = %d" % t]
        for name, v32, v64, dd in zip("wmv", r32, r64, d):
            mx, rms, exact = A.errors(v32, v64, dd)
            assert exact, (t, name)
            out[k + name + "64"] = v64[rows]
            out[k + "floor_" + name] = np.asarray([mx, rms], np.float64)
            line.append("%s: max %.3g rms %.3g (D = 0 on %d)" % (name, mx, rms, int((dd == 0).sum())))
        print("  ".join(line))
    path = os.path.join(HERE, "adam_step.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
