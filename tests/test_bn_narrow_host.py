"""CPU tests of the plan options "bn_split_narrow" and "fuse_bn_pool" through the C ABI (no device): batch-statistics BatchNorm on
the split-f16 kernels (bn_batch_stats + bn_batch_split, precision 1) extended to YOLOv3-tiny's kind of graph — a BatchNorm conv
with 16 input channels on a raw-sum instance of a narrow tile, a 16-filter BatchNorm stem on the raw-sum instance of the split
stem, and the 2x2 / stride-2 max-pool that alone reads a BatchNorm conv inside its normalise kernel.  Without the mode the options
are inert.  Also: the float64 model of tests/bn_narrow_model.py and the layer-local gate catch three planted defects on the CPU
(what the GPU test then holds the kernels to)."""
import ctypes as C
import json

import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from oracle import darknet_ref as O
from bn_narrow_model import BY_NAME, MUTANTS, NARROW, NARROW_OPTIONS, cpu_stored, narrow_layer_model, pool_record
from conv_probes import FAMILIES, ProbePlan, accepted_ids, launch_of_layer
from f16s3_emulation import floors, gate, residual
from test_bn_split_host import _describe, _f, _info, _kernel_name, _launches, _opt, _plan, _snapshot

RTOD_E_ARG, RTOD_E_CFG, RTOD_E_STATE = -1, -3, -4
LK_CONV, LK_MAXPOOL, LK_STEM = 0, 4, 7
EPI_RAW = 16
MODE = ("narrow_cin", "stem_pool", "bn_batch_stats", "bn_batch_split", "bn_split_narrow")
NAMES = [p.name for p in NARROW]


def _mode_plan(text, res, max_batch=8, skip=(), extra=()):
    h = _plan(text, res, max_batch)
    for o in MODE:
        if o not in skip:
            assert _opt(h, o) == 0, (o, _ffi.last_error())
    for o, v in extra:
        assert _opt(h, o, v) == 0, (o, _ffi.last_error())
    return h


def _fused(h):
    return {L["index"]: L["fused_into"] for L in json.loads(_describe(h))["layers"] if L["type"] == "convolutional" and L["bn"]}


def test_the_option_exists():
    """Fails on a library without the feature: an unknown option name is RTOD_E_ARG."""
    h = _plan(cfgs.mini_cfg(), 64)
    assert _opt(h, "bn_split_narrow") == 0, _ffi.last_error()
    assert _opt(h, "fuse_bn_pool", 0) == 0, _ffi.last_error()
    _ffi.lib().rtod_plan_destroy(h)


def test_yolov3_tiny_416_is_accepted_in_both_call_orders():
    lib = _ffi.lib()
    text = cfgs.yolov3_tiny_cfg()
    snaps = []
    for order in ("options first", "precision first"):
        h = _plan(text, 416)
        if order == "options first":
            for o in MODE:
                assert _opt(h, o) == 0, (o, _ffi.last_error())
            assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
        else:
            assert _opt(h, "narrow_cin") == 0                                 # (tiny needs it for precision 1 at all)
            assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
            for o in ("stem_pool", "bn_split_narrow", "bn_batch_split", "bn_batch_stats"):   # bn_batch_stats completes the combination
                assert _opt(h, o) == 0, (o, _ffi.last_error())
        snap = _snapshot(h)
        snaps.append(snap)
        d = json.loads(snap[0])
        assert _fused(h) == {0: 1, 2: 3, 4: 5, 6: 7, 8: -1, 10: -1, 12: -1, 13: -1, 14: -1, 18: -1, 21: -1}
        # the raw-sum scratch: every BatchNorm conv with its own row stride — Cout rounded up to 8 on the stem and the narrow tiles
        # (layers 0 and 2), Npad on the others
        bn = {L["index"]: L for L in d["layers"] if L["type"] == "convolutional" and L["bn"]}
        row = lambda L: (L["cout"] + 7) // 8 * 8 if L["index"] == 0 or L["cin"] == 16 else (L["cout"] + 127) // 128 * 128
        want = max(4 * 8 * L["hout"] * L["wout"] * row(L) for L in bn.values())
        assert d["bn_batch_split"] is True and d["bn_raw_bytes"] == want == 4 * 8 * 416 * 416 * 16
        kinds = [_f(l, "kind") for l in snap[1]]
        assert kinds[0] == LK_STEM and 1 not in kinds                          # the split stem reads NCHW: no pack launch
        for l in snap[1]:
            layer, kind = _f(l, "layer"), _f(l, "kind")
            if kind == LK_MAXPOOL and layer in (1, 3, 5, 7):
                assert _f(l, "bytes_per_frame") == 0, l                        # the entry stays and enqueues nothing
            if kind == LK_MAXPOOL and layer in (9, 11):
                assert _f(l, "bytes_per_frame") > 0, l
            if kind == LK_CONV and layer == 2:
                v = _f(l, "variant")
                assert v - 100 in FAMILIES["narrow"] and l[-1] == _kernel_name(v, EPI_RAW) and "conv_c16" in l[-1] and ", 16>" in l[-1], l
            if kind == LK_CONV and layer in bn and layer > 2:
                assert l[-1] == _kernel_name(_f(l, "variant"), EPI_RAW), l
        lib.rtod_plan_destroy(h)
    assert snaps[0] == snaps[1]


def test_no_conv_is_fused_with_fuse_bn_pool_off_or_keep_all_layers():
    lib = _ffi.lib()
    for text, res in ((cfgs.yolov3_tiny_cfg(), 416), (cfgs.bn_pool_mini_cfg(), 64)):
        h = _mode_plan(text, res, extra=(("fuse_bn_pool", 0),))
        assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
        assert set(_fused(h).values()) == {-1}
        assert all(_f(l, "bytes_per_frame") > 0 for l in _launches(h) if _f(l, "kind") == LK_MAXPOOL)
        lib.rtod_plan_destroy(h)
        h = _mode_plan(text, res)
        assert lib.rtod_plan_set_keep_all_layers(h, 1) == 0
        assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
        assert set(_fused(h).values()) == {-1}
        lib.rtod_plan_destroy(h)


def test_bn_pool_mini_cfg_fuses_what_the_rule_names():
    lib = _ffi.lib()
    for res in (64, 40):
        h = _mode_plan(cfgs.bn_pool_mini_cfg(res, res), res, 3)
        assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
        d = json.loads(_describe(h))
        # stem, Cin-16 conv, 96-filter conv: fused; 12 is read by its pool and a route, 15's pool has stride 1
        assert _fused(h) == {0: 1, 2: 3, 4: 5, 6: -1, 8: -1, 10: -1, 12: -1, 15: -1}
        L = d["layers"]
        assert L[5]["coff"] == 32 and L[5]["buf"] == L[7]["buf"] == L[6]["buf"]      # the pooled map lands in a concat slice at coff > 0
        assert L[8]["cout"] == 24 and L[4]["cout"] == 96                            # one-stage statistics (256 % (Cout / 4) != 0)
        assert L[17]["fused_into"] == 18 and res // L[17]["hout"] == 8              # a linear head with fused decode at stride 8
        assert L[16]["type"] == "maxpool" and L[16]["stride"] == 1 and L[13]["stride"] == 2
        c, hh, ww = C.c_int(), C.c_int(), C.c_int()
        assert lib.rtod_plan_layer_shape(h, 4, C.byref(c), C.byref(hh), C.byref(ww)) == RTOD_E_STATE
        assert lib.rtod_plan_layer_shape(h, 12, C.byref(c), C.byref(hh), C.byref(ww)) == 0
        lib.rtod_plan_destroy(h)


def test_without_the_option_the_refusals_are_as_before():
    lib = _ffi.lib()
    for narrow in (0, 1):
        h = _plan(cfgs.yolov3_tiny_cfg(), 416)
        assert _opt(h, "narrow_cin", narrow) == 0
        assert _opt(h, "bn_batch_stats") == 0 and _opt(h, "bn_batch_split") == 0
        assert lib.rtod_plan_set_precision(h, 1) == RTOD_E_CFG
        assert _ffi.last_error() == ("precision f16s3 with bn_batch_stats + bn_batch_split: layer 2 is a narrow BatchNorm conv (Cin=16: no raw-sum "
                                     "instance); use fp32"), _ffi.last_error()
        lib.rtod_plan_destroy(h)
    h = _plan(cfgs.yolov3_tiny_cfg(), 416)
    for o in ("narrow_cin", "stem_pool", "bn_batch_stats", "bn_batch_split"):
        assert _opt(h, o) == 0
    assert lib.rtod_plan_set_precision(h, 1) == RTOD_E_CFG
    assert _ffi.last_error() == ("precision f16s3 with bn_batch_stats + bn_batch_split: option stem_pool is not supported in that mode (layer 0 would "
                                 "run a kernel without a raw-sum instance)"), _ffi.last_error()
    assert _opt(h, "bn_split_narrow") == 0 and lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
    assert _opt(h, "bn_split_narrow", 0) == RTOD_E_CFG                        # ... and taking it back is refused, the plan stays
    assert _fused(h)[0] == 1
    lib.rtod_plan_destroy(h)
    # with the option but without narrow_cin a 16-channel conv is what it is in an eval plan: not expressible
    h = _mode_plan(cfgs.yolov3_tiny_cfg(), 416, skip=("narrow_cin",))
    assert lib.rtod_plan_set_precision(h, 1) == RTOD_E_CFG and "Cin=16" in _ffi.last_error()
    lib.rtod_plan_destroy(h)


def test_with_the_option_the_other_refusals_stay_and_leave_the_plan_usable():
    lib = _ffi.lib()
    text = cfgs.yolov3_tiny_cfg()
    # plain f16
    h = _mode_plan(text, 416)
    assert lib.rtod_plan_set_precision(h, 2) == RTOD_E_CFG and "bn_batch_stats" in _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 1) == 0 and _fused(h)[0] == 1
    lib.rtod_plan_destroy(h)
    h = _mode_plan(text, 416, skip=("bn_batch_stats",))
    assert lib.rtod_plan_set_precision(h, 2) == 0
    assert _opt(h, "bn_batch_stats") == RTOD_E_CFG                             # the other order
    assert "bn_raw_bytes" not in _describe(h)
    lib.rtod_plan_destroy(h)
    # K-sliced convs, in either order
    h = _mode_plan(text, 416, extra=(("k_slices_split", 1),))
    assert lib.rtod_plan_set_precision(h, 1) == RTOD_E_CFG and "k_slices_split" in _ffi.last_error()
    assert _opt(h, "k_slices_split", 0) == 0 and lib.rtod_plan_set_precision(h, 1) == 0
    assert _opt(h, "k_slices_split") == RTOD_E_CFG and "k_slices_split" in _ffi.last_error()
    assert _fused(h) == {0: 1, 2: 3, 4: 5, 6: 7, 8: -1, 10: -1, 12: -1, 13: -1, 14: -1, 18: -1, 21: -1}
    lib.rtod_plan_destroy(h)
    # a BatchNorm conv with a fused head decode
    nout = 3 * 8
    L = cfgs._net(64, 64) + cfgs._conv(16, 3, 1) + cfgs._maxpool(2, 2) + cfgs._conv(32, 3, 2) + cfgs._conv(32, 3, 2)
    L += cfgs._conv(nout, 1, 1, bn=True, act="linear") + cfgs._yolo((0, 1, 2), cfgs._ANCHORS_V3, 9, 3)
    h = _mode_plan("\n".join(L) + "\n", 64)
    assert lib.rtod_plan_set_precision(h, 1) == RTOD_E_CFG and "fused head decode" in _ffi.last_error()
    assert lib.rtod_plan_set_precision(h, 0) == 0
    lib.rtod_plan_destroy(h)
    # a rectangular plan has no batch-statistics mode at all
    h = _plan(cfgs.yolov3_tiny_cfg(416, 608), 416, rect_w=608)
    assert _opt(h, "narrow_cin") == 0 and _opt(h, "bn_split_narrow") == 0 and _opt(h, "bn_batch_split") == 0
    assert _opt(h, "bn_batch_stats") == RTOD_E_ARG
    assert lib.rtod_plan_set_precision(h, 1) == 0 and "bn_raw_bytes" not in _describe(h)
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("net", ["yolov3", "yolov3-tiny", "stem_pool_mini"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_without_bn_batch_stats_the_options_are_inert(net, mode):
    """Describe JSON, every field of every launch, kernel names, packed-weight and arena sizes, and the accepted tile ids of every
    conv launch equal those of a plan that never saw the options."""
    lib = _ffi.lib()
    text, res = {"yolov3": (cfgs.yolov3_cfg(), 416), "yolov3-tiny": (cfgs.yolov3_tiny_cfg(), 416), "stem_pool_mini": (cfgs.stem_pool_mini_cfg(), 64)}[net]
    got = []
    for with_options in (False, True):
        h = _plan(text, res)
        if net != "yolov3":
            assert _opt(h, "narrow_cin") == 0 and _opt(h, "stem_pool") == 0
        if with_options:
            assert _opt(h, "bn_split_narrow") == 0 and _opt(h, "fuse_bn_pool", 0) == 0 and _opt(h, "bn_batch_split") == 0, _ffi.last_error()
        rc = lib.rtod_plan_set_precision(h, mode)
        snap = _snapshot(h)
        tiles = []
        if mode:
            n = _info(h).n_launches
            convs = [i for i, l in enumerate(snap[1]) if _f(l, "kind") == LK_CONV and _f(l, "variant") >= 100]
            if net == "yolov3":                                                # 75 conv launches x 170 ids: the first launch of every kind of default tile
                first = {}                                                     # (generic, band, 1x1 slab, ... by tens of the id) and every head conv
                for i in convs:
                    first.setdefault(((_f(snap[1][i], "variant") - 100) // 10, _f(snap[1][i], "ksize"), _f(snap[1][i], "stride")), i)
                convs = sorted(set(first.values()) | {i for i in convs if _f(snap[1][i], "fused_decode")})
                assert len(convs) >= 6
            tiles = [accepted_ids(lib, h, n, i, 8) for i in convs]
        got.append((rc, snap, tiles))
        lib.rtod_plan_destroy(h)
    assert got[0][0] == 0 and got[0] == got[1]
    assert "bn_raw_bytes" not in got[1][1][0]


def test_yolov3_raw_scratch_is_unchanged():
    lib = _ffi.lib()
    for narrow in (0, 1):
        h = _plan(cfgs.yolov3_cfg(608, 608), 608)
        assert _opt(h, "bn_batch_stats") == 0 and _opt(h, "bn_batch_split") == 0 and _opt(h, "bn_split_narrow", narrow) == 0
        assert lib.rtod_plan_set_precision(h, 1) == 0, _ffi.last_error()
        assert json.loads(_describe(h))["bn_raw_bytes"] == 1514143744
        lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("name", NAMES)
def test_tile_table_of_a_narrow_batchnorm_conv_is_the_narrow_family(name):
    p = BY_NAME[name]
    lib = _ffi.lib()
    plan = ProbePlan(p, 1)
    try:
        infos = plan.launches()
        assert infos[0].kind == LK_STEM                                        # the 16-filter split stem
        launch = launch_of_layer(infos, p.conv_layer)
        got = accepted_ids(lib, plan.h, plan.n, launch, p.B)
        assert got == list(FAMILIES["narrow"]), (name, got)
        default = infos[launch].variant - 100
        assert default in got
        buf = C.create_string_buffer(256)
        assert lib.rtod_plan_launch_kernel_name(plan.h, launch, buf, 256) == 0
        assert buf.value.decode() == _kernel_name(100 + default, EPI_RAW)
        assert lib.rtod_plan_set_option(plan.h, b"force_f16s3_variant", 0) == 0      # an illegal id falls to the default
        assert plan.launches()[launch].variant == 100 + default
    finally:
        plan.close()


def test_kernel_names_of_the_raw_instances():
    for v in FAMILIES["narrow"]:
        raw, plain, f16 = _kernel_name(100 + v, EPI_RAW), _kernel_name(100 + v, 0), _kernel_name(100 + v, 8)
        assert raw and "conv_c16_f16s3_kernel" in raw and raw.endswith(", 16>(rtod::ConvArgs, int, int)")
        assert len({raw, plain, f16}) == 3


_cache = {}


def _pool_setup():
    """bn_pool_mini_cfg at 64x64, B = 1 on the CPU: oracle, input, the model's stored layers up to the pool of the Cin-16 conv."""
    if not _cache:
        text = cfgs.bn_pool_mini_cfg(64, 64)
        ref = O.RefDarknet(text, 64)
        ref.load_weight_stream(synth.synth_weights(ref.ir))
        x = torch.from_numpy(synth.synth_frames(1, 64, seed=9))
        with torch.no_grad():
            _cache["v"] = (ref, x, cpu_stored(ref, x, 3))
    return _cache["v"]


@pytest.mark.parametrize("layer", [0, 2])
def test_the_gate_catches_planted_defects_on_the_cpu(layer):
    """The 16-filter split stem (layer 0) and the Cin-16 conv (layer 2) of bn_pool_mini_cfg with their pools, from the model's own
    stored inputs: every float32 reference passes the gate on the full-resolution layer and on the pooled pair, the unmutated model
    is the zero residual, and each planted defect that changes a bit of the layer or of its pooled pair is caught there (all three on layer 0)."""
    ref, x, stored = _pool_setup()
    L, prm = ref.ir.layers[layer], ref.params[layer]
    with torch.no_grad():
        rec = narrow_layer_model(L, prm, stored[layer - 1], None, references=True, split_stem=True, pooled=True)
        prec = pool_record(rec)
        fl, pfl = floors(rec), floors(prec)
        for k in rec["refs"]:
            assert gate(residual(rec["refs"][k], rec), fl)[0] and gate(residual(prec["refs"][k], prec), pfl)[0], (layer, k)
        same = narrow_layer_model(L, prm, stored[layer - 1], None, split_stem=True, pooled=True)
        assert gate(residual(same["model"], rec), fl)[0] and gate(residual(same["pool_model"], prec), pfl)[0]
        assert torch.equal(same["pool_model"], torch.nn.functional.max_pool2d(rec["model"], 2, 2))
        for mut in MUTANTS:
            if mut == "stem_lo_dropped" and layer != 0:
                continue
            bad = narrow_layer_model(L, prm, stored[layer - 1], None, mutant=mut, split_stem=True, pooled=True)
            if mut == "pool_hi_only" and torch.equal(bad["pool_model"], rec["pool_model"]):
                # the defect shows only in a window where two values share the hi half and a later one has the larger lo.  Layer 0's
                # 16384 windows over a smooth image hold such windows; layer 2's 8192 hold none, and the mutant is the model there
                assert layer == 2
                continue
            ok_l, q_rms, q_max = gate(residual(bad["model"], rec), fl)
            ok_p, p_rms, p_max = gate(residual(bad["pool_model"], prec), pfl)
            print("MUTANT %s on layer %d: layer rms %.1f F_rms max %.1f F_max | pooled rms %.1f F_rms max %.1f F_max" % (mut, layer, q_rms, q_max, p_rms, p_max))
            assert not (ok_l and ok_p), (layer, mut)
            if mut == "pool_hi_only":
                assert ok_l and not ok_p                                       # a defect of the pool alone


def test_probe_models_run_on_the_cpu():
    """Every narrow probe builds, its conv under test is layer 1 behind the split stem, and the model's float32 references pass the gate."""
    from conv_probes import setup
    for p in NARROW:
        ref, wts, x = setup(p)
        assert dict(p.options) == dict(NARROW_OPTIONS) and p.conv_layer == 1 and ref.ir.layers[1].cin == 16
        with torch.no_grad():
            a = narrow_layer_model(ref.ir.layers[0], ref.params[0], x, None, split_stem=True)["model"]
            rec = narrow_layer_model(ref.ir.layers[1], ref.params[1], a, None, references=True)
        fl = floors(rec)
        for k, v in rec["refs"].items():
            assert gate(residual(v, rec), fl)[0], (p.name, k)
