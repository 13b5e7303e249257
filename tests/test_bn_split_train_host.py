"""Host tests (no GPU) of training under batch statistics on the split-f16 kernels: a plan with precision 1 (f16s3), options
bn_batch_stats + bn_batch_split, the keep option of a scope and keep_bn_inputs.  What the plan decides before anything touches the
device: which combinations it accepts (in both orders of the calls), that its listings are the f16s3 eval plan's, where the kept
raw sums live, and which refusals stay.

The twin of the buffer test is the f16s3 EVAL plan with the same keep option: the arena of a batch-trained plan is assigned as if the
kept raw sums were not there, and the keep options are inert on a batch-statistics plan without keep_bn_inputs (nothing is trainable
there, as before), so that plan keeps less alive and is no twin."""
import ctypes as C

import pytest

from head_grad_cases import describe, pack, plan
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from scope_grad_cases import KEEP, plan_list

SPLIT = [("bn_batch_split", 1), ("bn_batch_stats", 1)]              # (bn_batch_split first: bn_batch_stats alone is refused on an f16s3 plan)
KEPT = SPLIT + [("keep_bn_inputs", 1)]
LISTINGS = [("rtod_plan_head_blocks", 3), ("rtod_plan_neck_layers", 2), ("rtod_plan_trainable_layers", 2), ("rtod_plan_full_layers", 2)]
MINI = cfgs.mini_cfg(64, 64)
MAX_BATCH = 4
SCOPES = sorted(KEEP)
SCOPES_ORDER = ["blocks", "neck", "backbone", "full"]              # the order of LISTINGS


def _keep(scope):
    """The keep option of the scope; "full" with layer 0 on its generic layout, the one on which the listings name it."""
    return list(KEEP[scope].items()) + ([("stem_kernel", 0)] if scope == "full" else [])


def _listings(h):
    return [plan_list(entry, h, columns) for entry, columns in LISTINGS]


def _listed(h, scope):
    rows = _listings(h)[SCOPES_ORDER.index(scope)]
    return [r[1] for r in rows if r[1] >= 0] if scope == "blocks" else [r[0] for r in rows]


def _set(h, options):
    for name, value in options:
        rc = _ffi.lib().rtod_plan_set_option(h, name.encode(), int(value))
        if rc:
            return rc
    return 0


@pytest.mark.parametrize("scope", SCOPES)
def test_the_plan_accepts_keep_bn_inputs_in_both_call_orders(scope):
    lib = _ffi.lib()
    first = plan(MINI, 64, MAX_BATCH, 1, _keep(scope) + KEPT)           # options, then the precision
    second = plan(MINI, 64, MAX_BATCH, 1)                              # the precision, then the options
    assert _set(second, _keep(scope) + KEPT) == 0, _ffi.last_error()
    d = describe(first)
    assert d == describe(second)
    assert d["bn_batch_split"] is True and d["bn_batch_trained"] == "split" and d["bn_input_bytes"] > 0
    # the mark is the batch-trained split plan's alone
    for options, precision in ((_keep(scope) + SPLIT, 1), (_keep(scope), 1), (_keep(scope) + [("bn_batch_stats", 1), ("keep_bn_inputs", 1)], 0)):
        other = plan(MINI, 64, MAX_BATCH, precision, options)
        assert "bn_batch_trained" not in describe(other)
        lib.rtod_plan_destroy(other)
    for h in (first, second):
        lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("scope", SCOPES)
def test_listings_buffers_and_arena_against_the_eval_plan(scope):
    lib = _ffi.lib()
    ev, on, off = plan(MINI, 64, MAX_BATCH, 1, _keep(scope)), plan(MINI, 64, MAX_BATCH, 1, _keep(scope) + KEPT), plan(MINI, 64, MAX_BATCH, 1, _keep(scope) + SPLIT)
    want = _listings(ev)
    assert _listings(on) == want and all(len(rows) for rows in want), scope
    assert all(conv == -1 for _, conv, _ in _listings(off)[0]) and _listings(off)[1:] == [[], [], []]       # as before: nothing is trainable without the option
    listed = _listed(on, scope)
    if scope == "full":
        assert listed[0] == 0                                          # layer 0 on its generic layout
    d_ev, d_on, d_off = describe(ev), describe(on), describe(off)
    # every buffer of the eval plan has its twin: same shape, same interval, same offset
    n = len(d_ev["bufs"])
    assert d_on["bufs"][:n] == d_ev["bufs"]
    # ... and the option changes no launch and no layer of the batch-statistics plan (the eval plan differs there: its stem kernel)
    assert d_on["layers"] == d_off["layers"] and d_on["n_launches"] == d_off["n_launches"]
    # behind them one buffer per listed conv, in layer order: rows of Npad floats (what every raw-sum tile family and the normalise
    # kernel take as raw_ld), one after the other, never reused
    shape = {L.index: L for L in build_ir(parse_cfg_text(MINI), 64).layers}
    extra = d_on["bufs"][n:]
    assert len(extra) == len(listed)
    at = d_ev["arena_floats"]
    for b, c in zip(extra, listed):
        L = shape[c]
        assert (b["C"], b["H"], b["W"]) == (-(-L.cout // 128) * 128, L.hout, L.wout) and b["offset"] == at and b["last"] == len(d_on["layers"]), (scope, c, b)
        at += -(-b["floats_per_frame"] * MAX_BATCH // 64) * 64
    assert d_on["arena_floats"] == at and d_on["bn_input_bytes"] == 4 * (at - d_ev["arena_floats"])
    info_on, info_ev = _ffi.PlanInfo(), _ffi.PlanInfo()
    assert lib.rtod_plan_get_info(on, C.byref(info_on)) == 0 and lib.rtod_plan_get_info(ev, C.byref(info_ev)) == 0
    assert info_on.arena_bytes - info_ev.arena_bytes == d_on["bn_input_bytes"]
    for h in (ev, on, off):
        lib.rtod_plan_destroy(h)


def test_the_packed_image_does_not_depend_on_the_option():
    lib = _ffi.lib()
    w = synth.synth_weights(build_ir(parse_cfg_text(MINI), 64))
    on, off = plan(MINI, 64, MAX_BATCH, 1, _keep("backbone") + KEPT), plan(MINI, 64, MAX_BATCH, 1, _keep("backbone") + SPLIT)
    assert (pack(on, w) == pack(off, w)).all()
    for h in (on, off):
        lib.rtod_plan_destroy(h)


def test_the_refusals_that_stay_name_the_option_or_the_layer():
    lib, err = _ffi.lib(), _ffi.last_error
    keep = _keep("backbone")
    tiny = cfgs.pool_train_mini_cfg(64, 64, stem=16)
    # a missing split option, in either order of the calls: the plan stays as it was
    for options in ([("bn_batch_stats", 1), ("keep_bn_inputs", 1)], [("bn_batch_split", 1), ("keep_bn_inputs", 1)], [("keep_bn_inputs", 1)]):
        h = plan(MINI, 64, MAX_BATCH, 0, keep + options)
        before = describe(h)
        assert lib.rtod_plan_set_precision(h, 1) == -3 and "keep_bn_inputs" in err() and describe(h) == before, options
        lib.rtod_plan_destroy(h)
    h = plan(MINI, 64, MAX_BATCH, 1, keep + [("bn_batch_split", 1)])
    before = describe(h)
    assert lib.rtod_plan_set_option(h, b"keep_bn_inputs", 1) == -3 and "keep_bn_inputs" in err() and describe(h) == before
    lib.rtod_plan_destroy(h)
    # precision 2 in every case
    h = plan(MINI, 64, MAX_BATCH, 0, keep + KEPT)
    assert lib.rtod_plan_set_precision(h, 2) == -3 and "keep_bn_inputs" in err()
    assert lib.rtod_plan_set_precision(h, 1) == 0, err()
    # ... on the accepted plan: the K-sliced kernels have no raw-sum instance, the option that would remove one of the two is refused
    assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == -3 and "k_slices_split" in err()
    assert lib.rtod_plan_set_option(h, b"bn_batch_split", 0) == -3 and "keep_bn_inputs" in err()
    # the 16-filter stem and the narrow tiles (packers of their own): by option ...
    assert lib.rtod_plan_set_option(h, b"stem_pool", 1) == -3 and "stem_pool" in err()
    assert lib.rtod_plan_set_option(h, b"bn_split_narrow", 1) == -3 and "bn_split_narrow" in err()
    lib.rtod_plan_destroy(h)
    narrow = [("narrow_cin", 1), ("stem_pool", 1), ("bn_batch_split", 1), ("bn_split_narrow", 1), ("bn_batch_stats", 1)]
    h = plan(tiny, 64, MAX_BATCH, 1, list(KEEP["full"].items()) + narrow)      # legal without keep_bn_inputs (YOLOv3-tiny's forward)
    before = describe(h)
    assert lib.rtod_plan_set_option(h, b"keep_bn_inputs", 1) == -3 and "bn_split_narrow" in err() and "keep_bn_inputs" in err() and describe(h) == before
    lib.rtod_plan_destroy(h)
    # ... and by layer: a conv that reads 16 channels has no raw-sum instance without bn_split_narrow
    h = plan(tiny, 64, MAX_BATCH, 0, list(KEEP["full"].items()) + [("narrow_cin", 1)] + KEPT)
    ir = build_ir(parse_cfg_text(tiny), 64)
    thin = next(L.index for L in ir.layers if L.type == "convolutional" and L.index > 0 and L.cin == 16)
    assert lib.rtod_plan_set_precision(h, 1) == -3 and "layer %d" % thin in err() and "narrow" in err()
    lib.rtod_plan_destroy(h)
    # a rectangular plan has no batch statistics at all
    h = C.c_void_p()
    text = cfgs.mini_cfg(64, 96).encode()
    assert lib.rtod_plan_create_rect(text, len(text), 64, 96, MAX_BATCH, 0, C.byref(h)) == 0, err()
    assert lib.rtod_plan_set_option(h, b"bn_batch_split", 1) == 0 and lib.rtod_plan_set_option(h, b"bn_batch_stats", 1) == -1 and "rectangular" in err()
    lib.rtod_plan_destroy(h)
