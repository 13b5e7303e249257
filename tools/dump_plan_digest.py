#!/usr/bin/env python3
"""Characterisation digest of what a plan is and what it uploads, through the C ABI alone (no device, nothing launched).

For every case (cfg x option set x precision x keep_all_layers x weight set) it records
  * packed_floats and the SHA-256 of the packed weight image (rtod_plan_pack_weights: what rtod_plan_load_weights would upload);
  * the SHA-256 of the rtod_plan_describe text;
  * the SHA-256 of the rtod_launch_info records of every launch, reported at batch 8 (a plan of max_batch 8) and at batch 1 (a
    plan of max_batch 1), read field by field in declared order.
A case whose plan the library refuses records the kind of refusal instead.

Weight sets: "synth" is synth.synth_weights(ir) (fixed seed); "edge" is derived from it per conv (synth.conv_weight_slices):
output channel 0 all zeros (no maximum: pre-scale exponent 0), channel 1 scaled by 2^-40 (exponent clamped at 40; subnormal and
flushed halves), channel 2 by 2^+30, and - where the conv has a fourth channel - channel 3 by 2^+50, which is what carries a
channel maximum past 2^37 (exponent clamped at -24) and scaled weights past 65520 (f16 infinity).  BatchNorm parameters stay
as synthesised.

The cfg "mini_stem64" is cfgs.mini_cfg() with 64 filters in layer 0 (no cfg of the package has a 64-filter 3x3 stem).  The one
case of YOLOv3 608x608 (the benchmark's plan) carries synthetic weights only; its weight digest (synthesis, packing and hashing) takes about four seconds on a
CPU and is kept.

  python tools/dump_plan_digest.py                 full text of every case on stdout
  python tools/dump_plan_digest.py --case NAME     one case
  python tools/dump_plan_digest.py --coverage      which case covers which packing branch / option
  python tools/dump_plan_digest.py --json FILE     {case: digest} (tests/golden/plan_digest.json)

RTOD_LIB selects another build of the library (see _ffi.py); diff the full text of two builds to find the launch, the describe
field or the 64 Ki-float block of the image at which they differ.  tests/test_plan_digest_host.py compares the digests of the
built library with the committed ones.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from realtimeobjectdetection_amd import _ffi, cfgs, synth  # noqa: E402
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text  # noqa: E402

# every name rtod_plan_set_option accepts, with its default
OPTION_DEFAULTS = {
    "fuse_pointwise": 1, "ring_kernel": 1, "pwd_kernel": 1, "stem2_kernel": 1, "k_slices": 1, "bn_batch_stats": 0, "bn_batch_split": 0,
    "bn_split_narrow": 0, "fuse_bn_pool": 1, "k_slice_workgroups": 1, "k_slices_split": 0, "patch_kernel": 1, "stem_kernel": 1,
    "band_kernel": 1, "fuse_shortcut": 1, "fuse_decode": 1, "zero_copy_concat": 1, "narrow_cin": 0, "stem_pool": 0, "fuse_stem_pool": 1,
    "force_f16s3_variant": -1, "force_f32_variant": -1,
}
# packing branches and describe arms a case can cover (the --coverage table; the test wants each at least once)
BRANCHES = [
    "f32_panel_K<Kpad", "f32_stem28", "split_stem32", "split_stem64", "split_stem16", "split_generic", "split_narrow_odd_taps",
    "bn_folded", "bn_unfolded_f32", "bn_unfolded_split", "bn_unfolded_narrow", "plain_bias", "k_slices_split", "keep_all", "refused",
]


def _mini_stem64():
    return cfgs.mini_cfg().replace("filters=32", "filters=64", 1)


CFGS = {
    "mini": (cfgs.mini_cfg, 64, 64),
    "mini_stem64": (_mini_stem64, 64, 64),
    "mini_fallback": (cfgs.mini_fallback_cfg, 64, 64),
    "narrow_mini": (cfgs.narrow_mini_cfg, 64, 64),
    "stem_pool_mini": (cfgs.stem_pool_mini_cfg, 64, 64),
    "stem_pool_mini_40x56": (lambda: cfgs.stem_pool_mini_cfg(40, 56), 40, 56),
    "bn_pool_mini": (cfgs.bn_pool_mini_cfg, 64, 64),
    "kslice_mini": (cfgs.kslice_mini_cfg, 64, 64),
    "v5_style_mini": (cfgs.v5_style_mini_cfg, 128, 128),
    "tiny_416": (lambda: cfgs.yolov3_tiny_cfg(416, 416), 416, 416),
    "yolov3_608": (lambda: cfgs.yolov3_cfg(608, 608), 608, 608),
}
NARROW = [("narrow_cin", 1)]
STEMPOOL = NARROW + [("stem_pool", 1)]
BN_SPLIT = [("bn_batch_stats", 1), ("bn_batch_split", 1)]
BN_NARROW = STEMPOOL + BN_SPLIT + [("bn_split_narrow", 1)]
FOLD = ("bn_folded", "plain_bias")
# (cfg, option-set name, options, precision, keep_all_layers, weight sets, branches covered)
_CASES = [
    ("mini", "defaults", [], 0, 0, ("synth", "edge"), ("f32_stem28",) + FOLD),
    ("mini", "defaults", [], 1, 0, ("synth", "edge"), ("split_stem32", "split_generic") + FOLD),
    ("mini", "defaults", [], 2, 0, ("synth", "edge"), ("split_stem32", "split_generic") + FOLD),
    ("mini", "nostem", [("stem_kernel", 0)], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad",) + FOLD),
    ("mini", "nostem", [("stem_kernel", 0)], 1, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "split_generic") + FOLD),
    ("mini", "bn_stats", [("bn_batch_stats", 1)], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "bn_unfolded_f32", "plain_bias")),
    ("mini", "bn_split", BN_SPLIT, 1, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "bn_unfolded_split", "plain_bias")),
    ("mini", "bn_split", BN_SPLIT, 2, 0, ("synth",), ("refused",)),
    ("mini", "unfused", [("fuse_shortcut", 0)], 1, 0, ("synth",), ("refused",)),
    ("mini", "f32_nowg", [("k_slice_workgroups", 0)], 0, 0, ("synth",), ("f32_stem28",) + FOLD),
    ("mini", "tiles_off", [("fuse_pointwise", 0), ("ring_kernel", 0), ("pwd_kernel", 0), ("stem2_kernel", 0), ("patch_kernel", 0), ("band_kernel", 0)],
     1, 0, ("synth",), ("split_stem32", "split_generic") + FOLD),
    ("mini", "forced", [("force_f16s3_variant", 3)], 1, 0, ("synth",), ("split_stem32", "split_generic") + FOLD),
    ("mini", "defaults", [], 0, 1, ("synth",), ("keep_all", "f32_stem28") + FOLD),
    ("mini", "defaults", [], 1, 1, ("synth",), ("keep_all", "split_stem32", "split_generic") + FOLD),
    ("mini", "kslices", [("k_slices_split", 1)], 1, 0, ("synth",), ("k_slices_split", "split_generic") + FOLD),
    ("mini_stem64", "defaults", [], 0, 0, ("synth", "edge"), ("f32_stem28",) + FOLD),
    ("mini_stem64", "defaults", [], 1, 0, ("synth", "edge"), ("split_stem64", "split_generic") + FOLD),
    ("mini_fallback", "defaults", [], 0, 0, ("synth", "edge"), ("f32_stem28",) + FOLD),
    ("mini_fallback", "unfused", [("fuse_shortcut", 0), ("fuse_decode", 0), ("zero_copy_concat", 0), ("k_slices", 0), ("force_f32_variant", 2)], 0, 0,
     ("synth",), ("f32_stem28",) + FOLD),
    ("mini_fallback", "defaults", [], 1, 0, ("synth",), ("refused",)),
    ("narrow_mini", "defaults", [], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad",) + FOLD),
    ("narrow_mini", "defaults", [], 1, 0, ("synth",), ("refused",)),
    ("narrow_mini", "narrow", NARROW, 1, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("narrow_mini", "narrow", NARROW, 2, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("narrow_mini", "narrow", NARROW, 1, 1, ("synth",), ("keep_all", "split_narrow_odd_taps") + FOLD),
    ("stem_pool_mini", "narrow", NARROW, 1, 0, ("synth",), ("f32_panel_K<Kpad", "split_narrow_odd_taps") + FOLD),
    ("stem_pool_mini", "stempool", STEMPOOL, 0, 0, ("synth",), ("f32_panel_K<Kpad",) + FOLD),
    ("stem_pool_mini", "stempool", STEMPOOL, 1, 0, ("synth", "edge"), ("split_stem16", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("stem_pool_mini", "stempool", STEMPOOL, 2, 0, ("synth", "edge"), ("split_stem16", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("stem_pool_mini", "stempool_unfused", STEMPOOL + [("fuse_stem_pool", 0)], 1, 0, ("synth",), ("split_stem16",) + FOLD),
    ("stem_pool_mini", "stempool", STEMPOOL, 1, 1, ("synth",), ("keep_all", "split_stem16") + FOLD),
    ("stem_pool_mini_40x56", "stempool", STEMPOOL, 1, 0, ("synth",), ("split_stem16", "split_narrow_odd_taps") + FOLD),
    ("stem_pool_mini_40x56", "bn_stats", [("bn_batch_stats", 1)], 0, 0, ("synth",), ("refused",)),
    ("bn_pool_mini", "defaults", [], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad",) + FOLD),
    ("bn_pool_mini", "bn_stats", [("bn_batch_stats", 1)], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "bn_unfolded_f32", "plain_bias")),
    ("bn_pool_mini", "bn_split_only", STEMPOOL + BN_SPLIT, 1, 0, ("synth",), ("refused",)),
    ("bn_pool_mini", "bn_narrow", BN_NARROW, 1, 0, ("synth", "edge"), ("split_stem16", "split_narrow_odd_taps", "bn_unfolded_narrow", "plain_bias")),
    ("bn_pool_mini", "bn_narrow_unfused", BN_NARROW + [("fuse_bn_pool", 0)], 1, 0, ("synth",), ("split_stem16", "bn_unfolded_narrow", "plain_bias")),
    ("bn_pool_mini", "bn_narrow", BN_NARROW, 1, 1, ("synth",), ("keep_all", "bn_unfolded_narrow")),
    ("bn_pool_mini", "bn_narrow_nostempool", NARROW + BN_SPLIT + [("bn_split_narrow", 1)], 1, 0, ("synth",), ("f32_panel_K<Kpad", "bn_unfolded_narrow", "plain_bias")),
    ("kslice_mini", "defaults", [], 0, 0, ("synth",), ("f32_stem28",) + FOLD),
    ("kslice_mini", "defaults", [], 1, 0, ("synth", "edge"), ("split_stem32", "split_generic") + FOLD),
    ("kslice_mini", "kslices", [("k_slices_split", 1)], 1, 0, ("synth", "edge"), ("k_slices_split", "split_stem32", "split_generic") + FOLD),
    ("kslice_mini", "kslices", [("k_slices_split", 1)], 2, 0, ("synth",), ("k_slices_split", "split_generic") + FOLD),
    ("kslice_mini", "kslices_nowg", [("k_slices_split", 1), ("k_slice_workgroups", 0)], 1, 0, ("synth",), ("k_slices_split",) + FOLD),
    ("kslice_mini", "kslices_bn_split", BN_SPLIT + [("k_slices_split", 1)], 1, 0, ("synth",), ("refused",)),
    ("v5_style_mini", "defaults", [], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad",) + FOLD),
    ("v5_style_mini", "defaults", [], 1, 0, ("synth", "edge"), ("f32_panel_K<Kpad", "split_generic") + FOLD),
    ("v5_style_mini", "defaults", [], 2, 0, ("synth",), ("f32_panel_K<Kpad", "split_generic") + FOLD),
    ("tiny_416", "defaults", [], 0, 0, ("synth", "edge"), ("f32_panel_K<Kpad",) + FOLD),
    ("tiny_416", "narrow", NARROW, 1, 0, ("synth",), ("f32_panel_K<Kpad", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("tiny_416", "stempool", STEMPOOL, 1, 0, ("synth", "edge"), ("split_stem16", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("tiny_416", "stempool", STEMPOOL, 2, 0, ("synth",), ("split_stem16", "split_narrow_odd_taps", "split_generic") + FOLD),
    ("tiny_416", "bn_narrow", BN_NARROW, 1, 0, ("synth",), ("split_stem16", "bn_unfolded_narrow", "bn_unfolded_split", "plain_bias")),
    ("yolov3_608", "defaults", [], 1, 0, ("synth",), ("split_stem32", "split_generic") + FOLD),
]


def cases():
    """(name, cfg name, options, precision, keep_all_layers, weight set, branches) of every case, in a fixed order."""
    for cname, oname, opts, prec, keep, wsets, cov in _CASES:
        for ws in wsets:
            yield "%s/%s/p%d%s/%s" % (cname, oname, prec, "/keep_all" if keep else "", ws), cname, opts, prec, keep, ws, cov


_weights = {}


def weights(cname, wset):
    """The weight stream of a cfg: computed once, read-only."""
    if (cname, wset) not in _weights:
        gen, h, w = CFGS[cname]
        ir = build_ir(parse_cfg_text(gen()), h, w)
        if wset == "synth":
            out = synth.synth_weights(ir)
        else:
            out = weights(cname, "synth").copy()
            for L in ir.layers:
                if L.type != "convolutional":
                    continue
                a, b = synth.conv_weight_slices(ir)[L.index]
                blk = out[a:b].reshape(L.cout, -1)
                for ch, f in ((0, 0.0), (1, 2.0 ** -40), (2, 2.0 ** 30), (3, 2.0 ** 50)):
                    if ch < L.cout:
                        blk[ch] *= np.float32(f)
        out.setflags(write=False)
        _weights[(cname, wset)] = out
    return _weights[(cname, wset)]


def _refusal_kind(step, msg):
    for key, tag in (("needs a stand-alone", "standalone-kernel"), ("is not supported in that mode", "option-without-raw-sum"),
                     ("unsupported with bn_batch_stats", "bn-stats-precision"), ("rectangular plan", "bn-stats-rect"),
                     ("use fp32", "layer-shape")):
        if key in msg:
            return "%s:%s" % (step, tag)
    return "%s:?(%s)" % (step, msg)


def _make_plan(lib, cname, opts, prec, keep, max_batch):
    """(handle, None) or (None, kind of refusal)."""
    gen, height, width = CFGS[cname]
    t = gen().encode()
    h = C.c_void_p()
    if lib.rtod_plan_create_rect(t, len(t), height, width, max_batch, 0, C.byref(h)):
        return None, _refusal_kind("plan_create", _ffi.last_error())
    for name, value in opts:
        if lib.rtod_plan_set_option(h, name.encode(), value):
            kind = _refusal_kind("%s=%d" % (name, value), _ffi.last_error())
            lib.rtod_plan_destroy(h)
            return None, kind
    if lib.rtod_plan_set_precision(h, prec):
        kind = _refusal_kind("precision %d" % prec, _ffi.last_error())
        lib.rtod_plan_destroy(h)
        return None, kind
    if keep:
        assert lib.rtod_plan_set_keep_all_layers(h, 1) == 0, _ffi.last_error()
    return h, None


def _launch_lines(lib, h, tag):
    info = _ffi.PlanInfo()
    assert lib.rtod_plan_get_info(h, C.byref(info)) == 0
    li = _ffi.LaunchInfo()
    out = []
    for i in range(info.n_launches):
        assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
        out.append("%s launch %d: " % (tag, i) + " ".join("%s=%d" % (f, getattr(li, f)) for f, _ in _ffi.LaunchInfo._fields_))
    return out


def case_parts(cname, opts, prec, keep, wset):
    """The three texts of one case (describe, launch records, image) and packed_floats; or the kind of refusal."""
    lib = _ffi.lib()
    h, refused = _make_plan(lib, cname, opts, prec, keep, 8)
    if h is None:
        return {"refused": refused}
    try:
        need = C.c_size_t()
        assert lib.rtod_plan_describe(h, None, 0, C.byref(need)) == 0
        buf = C.create_string_buffer(need.value)
        assert lib.rtod_plan_describe(h, buf, need.value, None) == 0
        launches = _launch_lines(lib, h, "b8")
        h1, refused1 = _make_plan(lib, cname, opts, prec, keep, 1)
        assert h1 is not None, refused1
        launches += _launch_lines(lib, h1, "b1")
        lib.rtod_plan_destroy(h1)
        w = weights(cname, wset)
        n = C.c_size_t()
        assert lib.rtod_plan_pack_weights(h, None, 0, None, 0, C.byref(n)) == 0, _ffi.last_error()
        image = np.empty(n.value, np.float32)
        assert lib.rtod_plan_pack_weights(h, w.ctypes.data_as(C.c_void_p), w.size, image.ctypes.data_as(C.c_void_p), image.size, None) == 0, _ffi.last_error()
        info = _ffi.PlanInfo()
        assert lib.rtod_plan_get_info(h, C.byref(info)) == 0 and info.packed_weight_bytes == 4 * n.value
        return {"describe": buf.value.decode(), "launches": "\n".join(launches) + "\n", "image": image, "packed_floats": int(n.value)}
    finally:
        lib.rtod_plan_destroy(h)


def case_digest(cname, opts, prec, keep, wset):
    p = case_parts(cname, opts, prec, keep, wset)
    if "refused" in p:
        return p
    sha = lambda b: hashlib.sha256(b).hexdigest()
    return {"packed_floats": p["packed_floats"], "weights_sha256": sha(p["image"].tobytes()), "describe_sha256": sha(p["describe"].encode()),
            "launches_sha256": sha(p["launches"].encode())}


def case_text(cname, opts, prec, keep, wset):
    p = case_parts(cname, opts, prec, keep, wset)
    if "refused" in p:
        return "refused: %s\n" % p["refused"]
    blocks = ["image block %d crc32 %08x" % (i // 65536, zlib.crc32(p["image"][i:i + 65536].tobytes())) for i in range(0, p["image"].size, 65536)]
    return "packed_floats %d\n%s\n%s%s\n" % (p["packed_floats"], p["describe"].replace("},{", "},\n{"), p["launches"], "\n".join(blocks))


def coverage():
    """({branch: [case names]}, {option: [case names that set it to a non-default value]})."""
    br = {b: [] for b in BRANCHES}
    op = {o: [] for o in OPTION_DEFAULTS}
    for name, _cname, opts, _prec, keep, _ws, cov in cases():
        for b in cov:
            br[b].append(name)
        for o, v in opts:
            if v != OPTION_DEFAULTS[o]:
                op[o].append(name)
    return br, op


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", help="print this case only")
    ap.add_argument("--coverage", action="store_true", help="print which cases cover which packing branch and which option")
    ap.add_argument("--json", help="write the per-case digests to this file instead of printing the text")
    a = ap.parse_args()
    if a.coverage:
        br, op = coverage()
        for title, table in (("branch", br), ("option set to a non-default value", op)):
            print("%-36s cases" % title)
            for k, v in table.items():
                print("%-36s %d: %s" % (k, len(v), ", ".join(v[:4]) + (" ..." if len(v) > 4 else "")))
        return
    digests = {}
    for name, cname, opts, prec, keep, ws, _cov in cases():
        if a.case and name != a.case:
            continue
        if a.json:
            digests[name] = case_digest(cname, opts, prec, keep, ws)
        else:
            sys.stdout.write("=== %s\n%s" % (name, case_text(cname, opts, prec, keep, ws)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(digests, f, indent=0, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
