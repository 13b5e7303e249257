#!/usr/bin/env python3
"""Characterisation table of the split-f16 tile rules, through the C ABI alone (no device, no weights, nothing launched).

For every case (cfg x option set x precision) and every launch of its plan it prints
  * the variant and kernel name the plan reports with no forced id, at batch 8 and batch 1;
  * the variant and kernel name under every forced id 0 .. 169 (option force_f16s3_variant), at batch 8 and batch 1;
  * for every id 0 .. 169 whether a tile table with only that entry set is accepted by rtod_plan_set_tiles at batch 1 and 8
    (refusals are recorded by the kind of their error text).
A case whose plan the library refuses records the refusal text instead.

  python tools/dump_tile_rules.py                 full text of every case on stdout
  python tools/dump_tile_rules.py --case NAME     one case
  python tools/dump_tile_rules.py --json FILE     {case: {"sha256": ..., "launches": n}} (tests/golden/tile_rules.json)

RTOD_LIB selects another build of the library (see _ffi.py); diff the full text of two builds to find the launch and the id
at which they differ.  tests/test_tile_rules_host.py compares the hashes of the built library with the committed ones.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from realtimeobjectdetection_amd import _ffi, cfgs  # noqa: E402

IDS = range(170)
MAX_BATCH = 8

CFGS = [
    ("yolov3_608", lambda: cfgs.yolov3_cfg(608, 608), 608, 608),
    ("yolov3_416", lambda: cfgs.yolov3_cfg(416, 416), 416, 416),
    ("yolov3_416x608", lambda: cfgs.yolov3_cfg(416, 608), 416, 608),
    ("tiny_416", lambda: cfgs.yolov3_tiny_cfg(416, 416), 416, 416),
    ("v5s_640", lambda: cfgs.yolov5s_style_cfg(640, 640), 640, 640),
    ("mini", lambda: cfgs.mini_cfg(), 64, 64),
    ("narrow_mini", lambda: cfgs.narrow_mini_cfg(), 64, 64),
    ("stem_pool_mini", lambda: cfgs.stem_pool_mini_cfg(), 64, 64),
    ("kslice_mini", lambda: cfgs.kslice_mini_cfg(), 64, 64),
    ("v5_style_mini", lambda: cfgs.v5_style_mini_cfg(), 128, 128),
]
OPTION_SETS = [
    ("defaults", []),
    ("narrow", [("narrow_cin", 1)]),
    ("narrow_stempool", [("narrow_cin", 1), ("stem_pool", 1)]),
    ("kslices", [("k_slices_split", 1)]),
    ("kslices_nowg", [("k_slices_split", 1), ("k_slice_workgroups", 0)]),
    ("nopw", [("fuse_pointwise", 0)]),
    ("noband", [("band_kernel", 0)]),
    ("nopwd", [("pwd_kernel", 0)]),
]
PRECISIONS = (1, 2)


def cases():
    """(name, cfg text, height, width, options, precision) of every case, in a fixed order."""
    for cname, text, h, w in CFGS:
        for oname, opts in OPTION_SETS:
            for prec in PRECISIONS:
                yield "%s/%s/p%d" % (cname, oname, prec), text(), h, w, opts, prec


def _reported(lib, h, n):
    """'variant:kernel name' of every launch, at the batch the plan reports for (its last tile table's, else max_batch)."""
    out = []
    li = _ffi.LaunchInfo()
    buf = C.create_string_buffer(512)
    for i in range(n):
        assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
        rc = lib.rtod_plan_launch_kernel_name(h, i, buf, 512)
        out.append("%d:%s" % (li.variant, buf.value.decode() if rc == 0 else "ERROR " + _ffi.last_error()))
    return out


def _refusal_kind(msg):
    for key, tag in (("not a valid tile", "T"), ("needs more slice scratch", "S"), ("is not a split-f16 convolution", "C")):
        if key in msg:
            return tag
    return "?(" + msg + ")"


def case_text(text, height, width, opts, prec):
    """(printed text of one case, its launch count)."""
    lib = _ffi.lib()
    h = C.c_void_p()
    t = text.encode()
    lines = []
    rc = lib.rtod_plan_create_rect(t, len(t), height, width, MAX_BATCH, 0, C.byref(h))
    if rc:
        return "refused: plan_create: %s\n" % _ffi.last_error(), 0
    try:
        for name, value in opts:
            if lib.rtod_plan_set_option(h, name.encode(), value):
                return "refused: %s=%d: %s\n" % (name, value, _ffi.last_error()), 0
        if lib.rtod_plan_set_precision(h, prec):
            return "refused: precision %d: %s\n" % (prec, _ffi.last_error()), 0
        info = _ffi.PlanInfo()
        assert lib.rtod_plan_get_info(h, C.byref(info)) == 0
        n = info.n_launches
        empty = (C.c_int * n)(*([-1] * n))

        def both_batches():
            b8 = _reported(lib, h, n)                                   # no tile table: reported at max_batch
            assert lib.rtod_plan_set_tiles(h, 1, empty, n) == 0, _ffi.last_error()
            b1 = _reported(lib, h, n)                                   # an all-heuristic table of batch 1: reported at batch 1
            return b8, b1

        per_launch = [[] for _ in range(n)]
        for force in [-1] + list(IDS):
            assert lib.rtod_plan_set_option(h, b"force_f16s3_variant", force) == 0, _ffi.last_error()   # (re-plans: drops the tables)
            b8, b1 = both_batches()
            for i in range(n):
                per_launch[i].append("  force %3d: b8 %s | b1 %s" % (force, b8[i], b1[i]))
        assert lib.rtod_plan_set_option(h, b"force_f16s3_variant", -1) == 0
        table = (C.c_int * n)(*([-1] * n))
        for i in range(n):
            acc = {1: [], 8: []}
            for batch in (1, 8):
                for v in IDS:
                    table[i] = v
                    rc = lib.rtod_plan_set_tiles(h, batch, table, n)
                    acc[batch].append("+" if rc == 0 else _refusal_kind(_ffi.last_error()))
                table[i] = -1
            per_launch[i].append("  set_tiles b1: " + "".join(acc[1]))
            per_launch[i].append("  set_tiles b8: " + "".join(acc[8]))
        li = _ffi.LaunchInfo()
        for i in range(n):
            assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
            lines.append("launch %d layer %d kind %d" % (i, li.layer, li.kind))
            lines.extend(per_launch[i])
        return "\n".join(lines) + "\n", n
    finally:
        lib.rtod_plan_destroy(h)


def case_digest(text, height, width, opts, prec):
    out, n = case_text(text, height, width, opts, prec)
    return {"sha256": hashlib.sha256(out.encode()).hexdigest(), "launches": n}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", help="print this case only")
    ap.add_argument("--json", help="write the per-case hashes to this file instead of printing the text")
    a = ap.parse_args()
    digests = {}
    for name, text, h, w, opts, prec in cases():
        if a.case and name != a.case:
            continue
        out, n = case_text(text, h, w, opts, prec)
        digests[name] = {"sha256": hashlib.sha256(out.encode()).hexdigest(), "launches": n}
        if not a.json:
            sys.stdout.write("=== %s (%d launches)\n%s" % (name, n, out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(digests, f, indent=0, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
