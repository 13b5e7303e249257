"""CPU cross-check of the four views of a plan's run-time fused form (Plan::form / Plan::layer_form in csrc/plan_forward.cpp), through
the C ABI alone (no device, nothing launched): the rtod_plan_describe text, rtod_plan_layer_shape, the rtod_launch_info records and
rtod_plan_launch_kernel_name must agree with one another for every planned case of tools/dump_plan_digest.py.

"Run-time fused" is read off the describe text: a layer whose fused_into differs from what the same plan reports under
keep_all_layers, which switches every run-time fusion of stored layers off without planning again.

Narrowed where the library never behaved as the general statement says: rtod_plan_layer_shape refuses a run-time fused layer only
where a max-pool's kernel partner swallowed it (16-filter stem + pool, normalise + pool).  Layer 0 of the fused stem kernel (reported
fused into the conv of layer 1) keeps its arena buffer and its shape stays readable."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from realtimeobjectdetection_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_plan_digest", os.path.join(ROOT, "tools", "dump_plan_digest.py"))
dump_plan_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plan_digest)

LK_CONV, LK_MAXPOOL, LK_STEM = 0, 4, 7
RTOD_E_STATE = -4
# (cfg, option-set name, precision, keep_all_layers) -> (cfg, options, precision, keep_all_layers): the weight set does not matter here
PLANS = {(c[1], c[0].split("/")[1], c[3], c[4]): (c[1], c[2], c[3], c[4]) for c in dump_plan_digest.cases()}
_views = {}


def _view(key):
    """What the C ABI reports of one case, computed once: None if the plan is refused."""
    if key not in _views:
        lib = _ffi.lib()
        h, _refused = dump_plan_digest._make_plan(lib, *PLANS[key], 8)
        if h is None:
            _views[key] = None
            return None
        try:
            need = C.c_size_t()
            assert lib.rtod_plan_describe(h, None, 0, C.byref(need)) == 0
            buf = C.create_string_buffer(need.value)
            assert lib.rtod_plan_describe(h, buf, need.value, None) == 0
            info = _ffi.PlanInfo()
            assert lib.rtod_plan_get_info(h, C.byref(info)) == 0
            launches = []
            name = C.create_string_buffer(512)
            for i in range(info.n_launches):
                li = _ffi.LaunchInfo()
                assert lib.rtod_plan_get_launch(h, i, C.byref(li)) == 0
                assert lib.rtod_plan_launch_kernel_name(h, i, name, 512) == 0, _ffi.last_error()
                launches.append((li.kind, li.flops_per_frame, li.bytes_per_frame, name.value.decode()))
            c, hh, w = C.c_int(), C.c_int(), C.c_int()
            shape_rc = [lib.rtod_plan_layer_shape(h, i, C.byref(c), C.byref(hh), C.byref(w)) for i in range(info.n_layers)]
            _views[key] = {"layers": json.loads(buf.value.decode())["layers"], "launches": launches, "shape_rc": shape_rc,
                           "conv_flops": info.conv_flops_per_frame}
        finally:
            lib.rtod_plan_destroy(h)
    return _views[key]


def _planned(keys):
    return sorted(k for k in keys if _view(k) is not None)


def _twin(key):
    """The same case under keep_all_layers."""
    twin = key[:3] + (1,)
    PLANS.setdefault(twin, PLANS[key][:3] + (1,))
    return twin


ALL = sorted(PLANS)
FUSION_PAIRS = [(("stem_pool_mini", "stempool", 1, 0), ("stem_pool_mini", "stempool_unfused", 1, 0)),
                (("bn_pool_mini", "bn_narrow", 1, 0), ("bn_pool_mini", "bn_narrow_unfused", 1, 0)),
                (("mini", "defaults", 1, 0), ("mini", "tiles_off", 1, 0))]


def test_the_cases_reach_every_run_time_fusion():
    assert len(_planned(ALL)) >= 40
    fused = set()
    for key in _planned(ALL):
        v, k = _view(key), _view(_twin(key))
        fused |= {(L["type"], v["layers"][L["fused_into"]]["type"]) for L, K in zip(v["layers"], k["layers"]) if L["fused_into"] != K["fused_into"]}
        fused |= {"idle conv" for kind, flops, nbytes, _ in v["launches"] if kind == LK_CONV and not flops and not nbytes}
    assert fused == {("convolutional", "maxpool"), ("convolutional", "convolutional"), "idle conv"}


@pytest.mark.parametrize("key", ALL, ids=lambda k: "%s/%s/p%d%s" % (k[0], k[1], k[2], "/keep_all" if k[3] else ""))
def test_the_views_of_one_plan_agree(key):
    v = _view(key)
    if v is None:
        return                                                  # refused plan: tests/test_plan_digest_host.py pins the reason
    k = _view(_twin(key))
    layers = v["layers"]
    # rtod_plan_layer_shape: refused exactly where the describe text shows no buffer, or a conv that a max-pool's kernel swallowed
    for L, K, rc in zip(layers, k["layers"], v["shape_rc"]):
        r = L
        while r["alias_of"] >= 0:
            r = layers[r["alias_of"]]
        pooled_away = L["fused_into"] != K["fused_into"] and layers[L["fused_into"]]["type"] == "maxpool"
        assert rc == (RTOD_E_STATE if r["buf"] < 0 or pooled_away else 0), (L["index"], rc)
    # a launch that enqueues nothing has no kernel name
    for kind, flops, nbytes, name in v["launches"]:
        if kind in (LK_CONV, LK_STEM, LK_MAXPOOL) and flops == 0 and nbytes == 0:
            assert name == ""
    # the FLOPs of the network ride some launch, whichever fusions are active; keep_all_layers moves them without re-planning
    assert sum(l[1] for l in v["launches"]) == v["conv_flops"] == k["conv_flops"]
    assert len(v["launches"]) == len(k["launches"])


@pytest.mark.parametrize("a,b", FUSION_PAIRS, ids=lambda k: "%s/%s" % k[:2])
def test_a_fusion_switch_moves_costs_between_launches_only(a, b):
    va, vb = _view(a), _view(b)
    assert sum(l[1] for l in va["launches"]) == sum(l[1] for l in vb["launches"]) == va["conv_flops"] == vb["conv_flops"]
    assert len(va["launches"]) == len(vb["launches"])
    assert [l[:3] for l in va["launches"]] != [l[:3] for l in vb["launches"]]      # the pair really differs in form
