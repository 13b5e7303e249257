"""CPU tests of the plan option "k_slices_split" through the C ABI: with it a precision-1 (f16s3) or precision-2 (f16) plan forms
the K sum of its deep small-grid convolutions in slices, on the K-sliced tile family (conv_ks_f16s3.hip, tile ids 150 ...);
without it every plan is what it was, and exact-fp32 plans ignore it.

The rule is restated here from the layer shapes alone: a conv after layer 0 with Cin % 32 == 0, no fused head decode, outside
the fused-pointwise pairs, hout * wout <= 2704 and at least 8 K-chunks of 32 is sliced in slices of 9 (>= 32 chunks),
4 (>= 16) or 2 chunks.  Tile ids: 150 + 2 * tile + schedule (0: slices inside the workgroup, 1: one workgroup per slice);
rtod_launch_info.variant reports 100 + id like the other split families."""
import ctypes as C
import json

import pytest

from realtimeobjectdetection_amd import _ffi, cfgs

RTOD_E_ARG = -1
KS_BASE, KS_MODES = 150, 6
C16_BASE, C16_MODES = 140, 4
LK_CONV = 0
FIELDS = [f for f, _ in _ffi.LaunchInfo._fields_]


def _plan(text, res, max_batch=8):
    lib = _ffi.lib()
    h = C.c_void_p()
    t = text.encode()
    assert lib.rtod_plan_create(t, len(t), res, res, max_batch, 0, C.byref(h)) == 0, _ffi.last_error()
    return h


def _describe(h):
    lib = _ffi.lib()
    need = C.c_size_t()
    assert lib.rtod_plan_describe(h, None, 0, C.byref(need)) == 0
    b = C.create_string_buffer(need.value)
    assert lib.rtod_plan_describe(h, b, need.value, None) == 0
    return b.value.decode()


def _info(h):
    info = _ffi.PlanInfo()
    assert _ffi.lib().rtod_plan_get_info(h, C.byref(info)) == 0
    return info


def _launches(h):
    """Every field of every launch, and the kernel name the launch runs."""
    lib = _ffi.lib()
    out = []
    for i in range(_info(h).n_launches):
        li = _ffi.LaunchInfo()
        assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
        buf = C.create_string_buffer(256)
        assert lib.rtod_plan_launch_kernel_name(h, i, buf, 256) == 0, _ffi.last_error()
        out.append(tuple(getattr(li, f) for f in FIELDS) + (buf.value.decode(),))
    return out


def _field(launch, name):
    return launch[FIELDS.index(name)]


def _is_ks(variant):
    return KS_BASE <= variant - 100 < KS_BASE + KS_MODES


def _snapshot(h):
    return _describe(h), _launches(h), _info(h).packed_weight_bytes, _info(h).arena_bytes, _info(h).n_launches


def _rule(launches):
    """layer -> number of slices, from the launch list of the plan WITHOUT the option (precision 1: it shows the pointwise pairs)."""
    out, skip = {}, set()
    for i, l in enumerate(launches):
        if _field(l, "kind") == LK_CONV and _field(l, "fused_pointwise"):
            skip |= {_field(l, "layer"), _field(launches[i + 1], "layer")}
    for l in launches:
        if _field(l, "kind") != LK_CONV or _field(l, "layer") == 0 or _field(l, "layer") in skip:
            continue
        cin, k = _field(l, "cin"), _field(l, "ksize")
        nkc = k * k * cin // 32
        if cin % 32 or _field(l, "fused_decode") or _field(l, "hout") * _field(l, "wout") > 2704 or nkc < 8:
            continue
        per = 9 if nkc >= 32 else 4 if nkc >= 16 else 2
        out[_field(l, "layer")] = (nkc + per - 1) // per
    return out


def test_the_option_exists():
    """Fails on a library without the feature: an unknown option name is RTOD_E_ARG."""
    lib = _ffi.lib()
    h = _plan(cfgs.mini_cfg(), 64)
    assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0, _ffi.last_error()
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("res", [608, 416])
def test_yolov3_off_is_the_old_plan_and_on_slices_what_the_rule_names(res, mode):
    lib = _ffi.lib()
    text = cfgs.yolov3_cfg()
    never = _plan(text, res)
    assert lib.rtod_plan_set_precision(never, mode) == 0, _ffi.last_error()
    base = _snapshot(never)
    assert "k_slices" not in base[0]
    p1 = _plan(text, res)                                                # the rule reads the pointwise pairs off a precision-1 plan
    assert lib.rtod_plan_set_precision(p1, 1) == 0
    want = _rule(_launches(p1))
    lib.rtod_plan_destroy(p1)
    assert len(want) >= 30 and all(s >= 4 for s in want.values())

    for order in ("option first", "precision first"):
        h = _plan(text, res)
        if order == "option first":
            assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0, _ffi.last_error()
            assert lib.rtod_plan_set_precision(h, mode) == 0, _ffi.last_error()
        else:
            assert lib.rtod_plan_set_precision(h, mode) == 0, _ffi.last_error()
            assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0, _ffi.last_error()
        on = _snapshot(h)
        d = json.loads(on[0])
        assert {L["index"]: L["k_slices"] for L in d["layers"] if "k_slices" in L} == want
        assert on[2:] == base[2:]                                        # same packed bytes, arena and n_launches
        assert len(on[1]) == len(base[1])
        for a, b in zip(base[1], on[1]):
            layer = _field(a, "layer")
            if _field(a, "kind") == LK_CONV and layer in want:
                assert _is_ks(_field(b, "variant")) and "conv_ks_f16s3_kernel" in b[-1], b          # no band / ring / pwd / generic tile
                assert lib.rtod_conv_variant_name(_field(b, "variant")).decode().startswith("conv_ks_f16s3<")
                buf = C.create_string_buffer(256)
                epi = (1 if _field(b, "fused_residual") else 0) | (8 if mode == 2 else 0)
                assert lib.rtod_conv_kernel_name(_field(b, "variant"), epi, buf, 256) == 0 and buf.value.decode() == b[-1]
                for f in FIELDS:
                    if f != "variant":
                        assert _field(a, f) == _field(b, f), (layer, f)
            else:                                                        # heads, stem, pointwise pairs, large grids, short K: as they were
                assert a == b, (a, b)
                assert not _is_ks(_field(b, "variant"))
        # on -> off: the plan that never saw the option
        assert lib.rtod_plan_set_option(h, b"k_slices_split", 0) == 0
        assert _snapshot(h) == base
        lib.rtod_plan_destroy(h)
    off = _plan(text, res)
    assert lib.rtod_plan_set_option(off, b"k_slices_split", 0) == 0
    assert lib.rtod_plan_set_precision(off, mode) == 0
    assert _snapshot(off) == base
    lib.rtod_plan_destroy(off)
    lib.rtod_plan_destroy(never)


@pytest.mark.parametrize("net", ["yolov3", "tiny", "kslice_mini"])
def test_precision_0_ignores_the_option(net):
    lib = _ffi.lib()
    text, res = {"yolov3": (cfgs.yolov3_cfg(), 416), "tiny": (cfgs.yolov3_tiny_cfg(), 416), "kslice_mini": (cfgs.kslice_mini_cfg(), 64)}[net]
    got = []
    for opt in (None, 1):
        h = _plan(text, res)
        if opt is not None:
            assert lib.rtod_plan_set_option(h, b"k_slices_split", opt) == 0, _ffi.last_error()
            assert lib.rtod_plan_set_precision(h, 0) == 0
        got.append(_snapshot(h))
        lib.rtod_plan_destroy(h)
    assert got[0] == got[1] and "k_slices" not in got[1][0]


@pytest.mark.parametrize("mode", [1, 2])
def test_tiny_with_narrow_cin_and_stem_pool(mode):
    lib = _ffi.lib()
    plans = {}
    for on in (0, 1):
        h = _plan(cfgs.yolov3_tiny_cfg(), 416)
        for name in (b"narrow_cin", b"stem_pool"):
            assert lib.rtod_plan_set_option(h, name, 1) == 0, _ffi.last_error()
        assert lib.rtod_plan_set_option(h, b"k_slices_split", on) == 0, _ffi.last_error()
        assert lib.rtod_plan_set_precision(h, mode) == 0, _ffi.last_error()
        plans[on] = (json.loads(_describe(h)), _launches(h))
        lib.rtod_plan_destroy(h)
    want = _rule(plans[0][1])
    assert want == {6: 5, 8: 4, 10: 8, 12: 16, 13: 4, 14: 8, 18: 4, 21: 12}            # the 52x52 / 26x26 / 13x13 layers but the heads
    assert {L["index"]: L["k_slices"] for L in plans[1][0]["layers"] if "k_slices" in L} == want
    assert len(plans[0][1]) == len(plans[1][1])
    for a, b in zip(plans[0][1], plans[1][1]):
        layer, v = _field(b, "layer"), _field(b, "variant")
        if _field(b, "kind") == LK_CONV and layer in want:
            assert _is_ks(v), b
        else:
            assert a == b
        if _field(b, "kind") == LK_CONV and layer == 2:
            assert C16_BASE <= v - 100 < C16_BASE + C16_MODES                            # layer 2 stays narrow


def test_kslice_mini_plan_has_the_cases_its_gpu_test_was_written_for():
    lib = _ffi.lib()
    for res_h, res_w in ((64, 64), (40, 56)):
        h = C.c_void_p()
        t = cfgs.kslice_mini_cfg(res_h, res_w).encode()
        assert lib.rtod_plan_create_rect(t, len(t), res_h, res_w, 3, 0, C.byref(h)) == 0, _ffi.last_error()
        assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0
        for mode in (1, 2):
            assert lib.rtod_plan_set_precision(h, mode) == 0, _ffi.last_error()
            d = json.loads(_describe(h))
            Ls = d["layers"]
            # 9 chunks in slices of 2; 18 in slices of 4 (twice, one with the shortcut); 18; 8 in slices of 2; 99 and 36 in slices of 9
            assert {L["index"]: L["k_slices"] for L in Ls if "k_slices" in L} == {2: 5, 3: 5, 4: 5, 6: 5, 7: 4, 9: 11, 10: 4}
            assert Ls[4]["fused_into"] == 5 and Ls[11]["fused_into"] == 12
            assert Ls[7]["buf"] == Ls[8]["buf"] == Ls[6]["buf"] and Ls[7]["coff"] == 0 and Ls[6]["coff"] == 96 and d["bufs"][Ls[8]["buf"]]["C"] == 352
            assert Ls[7]["cout"] == 96 and Ls[7]["act"] == 0
            by_layer = {_field(l, "layer"): l for l in _launches(h) if _field(l, "kind") == LK_CONV}
            assert sorted(i for i, l in by_layer.items() if _is_ks(_field(l, "variant"))) == [2, 3, 4, 6, 7, 9, 10]
            assert _field(by_layer[4], "fused_residual") and _field(by_layer[11], "fused_decode")
            assert 100 <= _field(by_layer[1], "variant") < 250 and 100 <= _field(by_layer[11], "variant") < 250
            assert not any(_field(l, "fused_pointwise") for l in by_layer.values())
        lib.rtod_plan_destroy(h)


def test_tile_tables_keep_the_family_apart():
    lib = _ffi.lib()
    h = _plan(cfgs.yolov3_cfg(), 416)
    assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0
    assert lib.rtod_plan_set_precision(h, 1) == 0
    launches = _launches(h)
    n = len(launches)
    sliced = [i for i, l in enumerate(launches) if _is_ks(_field(l, "variant"))]
    i_s = [i for i in sliced if _field(launches[i], "cout") == 1024 and _field(launches[i], "ksize") == 3][0]    # 13x13, 16 slices
    i_u = [i for i, l in enumerate(launches) if _field(l, "kind") == LK_CONV and _field(l, "layer") == 5][0]     # 208x208: not sliced
    assert i_u not in sliced

    def table(**kw):
        t = [-1] * n
        for k, v in kw.items():
            t[int(k[1:])] = v
        return (C.c_int * n)(*t)

    for v in range(KS_BASE, KS_BASE + KS_MODES):
        assert lib.rtod_plan_set_tiles(h, 1, table(**{"i%d" % i_u: v}), n) == RTOD_E_ARG       # a family id on an unsliced layer
    for v in (0, 3, 57, 72, 95, 112, 140, KS_BASE + KS_MODES):
        assert lib.rtod_plan_set_tiles(h, 1, table(**{"i%d" % i_s: v}), n) == RTOD_E_ARG       # a foreign id on a sliced layer
    for mode in range(KS_MODES):
        t = table(**{"i%d" % i_s: KS_BASE + mode})
        assert lib.rtod_plan_set_tiles(h, 1, t, n) == 0, _ffi.last_error()
        back = (C.c_int * n)()
        assert lib.rtod_plan_get_tiles(h, 1, back, n) == n and list(back) == list(t)
        assert _field(_launches(h)[i_s], "variant") == 100 + KS_BASE + mode
    # one workgroup per slice at batch 8: 16 slices x 8 x 169 pixels x 1024 floats do not fit the 32 MB of slice panels
    assert lib.rtod_plan_set_tiles(h, 8, table(**{"i%d" % i_s: KS_BASE + 1}), n) == RTOD_E_ARG
    assert "scratch" in _ffi.last_error()
    assert lib.rtod_plan_set_tiles(h, 8, table(**{"i%d" % i_s: KS_BASE}), n) == 0
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("force", [0, 57, 72, 95, 112, 141, 150, 152, 153, 155, 156])
def test_forced_variants_stay_inside_and_outside_the_family(force, mode):
    lib = _ffi.lib()
    plans = {}
    for f in (-1, force):
        h = C.c_void_p()
        t = cfgs.kslice_mini_cfg().encode()
        assert lib.rtod_plan_create(t, len(t), 64, 64, 1, 0, C.byref(h)) == 0
        assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0
        assert lib.rtod_plan_set_option(h, b"force_f16s3_variant", f) == 0
        assert lib.rtod_plan_set_precision(h, mode) == 0, _ffi.last_error()
        plans[f] = _launches(h)
        lib.rtod_plan_destroy(h)
    in_family = KS_BASE <= force < KS_BASE + KS_MODES
    for a, b in zip(plans[-1], plans[force]):
        if _field(b, "kind") != LK_CONV or _field(b, "layer") == 0:
            continue
        va, vb = _field(a, "variant"), _field(b, "variant")
        assert _is_ks(va) == _is_ks(vb)                                   # a sliced layer keeps its family, no other layer enters it
        if _is_ks(vb):
            assert vb == (100 + force if in_family else va)
        elif in_family:
            assert vb == va                                               # a family id means nothing to an unsliced layer


def test_k_slice_workgroups_0_reports_the_in_workgroup_schedule():
    lib = _ffi.lib()
    for wg in (1, 0):
        h = _plan(cfgs.yolov3_cfg(), 416, max_batch=1)
        assert lib.rtod_plan_set_option(h, b"k_slices_split", 1) == 0
        assert lib.rtod_plan_set_option(h, b"k_slice_workgroups", wg) == 0
        assert lib.rtod_plan_set_option(h, b"force_f16s3_variant", KS_BASE + 3) == 0
        assert lib.rtod_plan_set_precision(h, 1) == 0
        got = {_field(l, "variant") for l in _launches(h) if _is_ks(_field(l, "variant"))}
        assert got == ({100 + KS_BASE + 3} if wg else {100 + KS_BASE + 2})
        lib.rtod_plan_destroy(h)
