"""Host tests of the backbone training path (BatchNorm frozen): rtod_plan_trainable_layers with and without option
keep_backbone_activations, what the option does to the plan (the three fusions held, the forward's launches those of the plan with them
switched off), the numpy references of the stride-2 kernels against float64 torch.autograd, the workspace sizes and the refusals of
rtod_conv_dgrad_s2 / rtod_conv_wgrad_s2 / rtod_grad_join, and the trainer's errors — all decided on the host.  The device is covered by
tests/test_backbone_grad_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from backbone_grad_cases import MINI_S2, S2_SHAPES, TRAINABLE, conv_dgrad_s2_ref, conv_wgrad_s2_ref, out_hw, trainable_layers
from block_grad_cases import conv_wgrad_slices
from head_grad_cases import describe, pack, plan
from neck_grad_cases import NECK, neck_layers
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer

F = np.float32
ONE = C.c_void_p(64)                                                  # never dereferenced: every refusal is decided on the host
OPT = [("keep_backbone_activations", 1)]
OFF3 = [("fuse_shortcut", 0), ("fuse_pointwise", 0), ("stem2_kernel", 0)]
fn = torch.nn.functional


# ---------------------------------------------------------------------------------------------- 1. rtod_plan_trainable_layers
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_trainable_layers_with_the_option(precision):
    lib = _ffi.lib()
    for net, text, res, base in (("mini", cfgs.mini_cfg(64, 64), 64, []), ("tiny", cfgs.yolov3_tiny_cfg(416, 416), 416, [("narrow_cin", 1)] if precision else [])):
        h = plan(text, res, 4, precision, base + OPT)
        got = trainable_layers(h)
        assert [c for c, _ in got] == TRAINABLE[net] and all(i == c - 1 for c, i in got), (net, precision, got)
        assert [c for c, _ in neck_layers(h)] == NECK[net]
        one = [(C.c_int * 1)() for _ in range(2)]
        assert lib.rtod_plan_trainable_layers(h, *one, 1) == len(got) and (one[0][0], one[1][0]) == got[0]
        assert lib.rtod_plan_trainable_layers(h, None, None, 1) == -1 and lib.rtod_plan_trainable_layers(None, None, None, 0) == -1
        lib.rtod_plan_destroy(h)
    # YOLOv3: every BatchNorm conv except layer 0, derived from the IR
    text = cfgs.yolov3_cfg(416, 416)
    ir = build_ir(parse_cfg_text(text), 416)
    want = [L.index for L in ir.layers if L.type == "convolutional" and L.bn and L.index > 0]
    h = plan(text, 416, 2, precision, OPT)
    assert [c for c, _ in trainable_layers(h)] == want and len(want) == 71
    assert [c for c, _ in neck_layers(h)] == NECK["yolov3"]
    lib.rtod_plan_destroy(h)
    # batch-statistics BatchNorm: nothing is folded, nothing is trainable
    h = plan(cfgs.mini_cfg(64, 64), 64, 4, 0, [("bn_batch_stats", 1)] + OPT)
    assert trainable_layers(h) == []
    lib.rtod_plan_destroy(h)


def test_neck_layers_do_not_depend_on_the_option_and_default_plans_hide_the_fused_convs():
    lib = _ffi.lib()
    text = cfgs.mini_cfg(64, 64)
    for precision in (0, 1, 2):
        off, on = plan(text, 64, 4, precision), plan(text, 64, 4, precision, OPT)
        assert neck_layers(off) == neck_layers(on) and [c for c, _ in neck_layers(on)] == NECK["mini"]
        got = [c for c, _ in trainable_layers(off)]
        assert 3 not in got and 7 not in got                         # their shortcuts run in their epilogues: nothing stores their own output
        assert set(NECK["mini"]) <= set(got) <= set(TRAINABLE["mini"])
        d = describe(off)["layers"]
        assert d[3]["fused_into"] == 4 and d[7]["fused_into"] == 8
        lib.rtod_plan_destroy(off)
        lib.rtod_plan_destroy(on)


# ---------------------------------------------------------------------------------------------- 2. the option: the plan with the three fusions off
def _resolve(layers, i):
    while layers[i]["alias_of"] >= 0:
        i = layers[i]["alias_of"]
    return i


def _launches(h):
    lib, out = _ffi.lib(), []
    for k in range(describe(h)["n_launches"]):
        li = _ffi.LaunchInfo()
        assert lib.rtod_plan_get_launch(h, k, C.byref(li)) == 0
        out.append(li)
    return out


def _split_plan_holds_the_fusions(text, res, precision):
    """Split-f16 / f16 plans.  The library refuses fuse_shortcut = 0 there on its own (no plan without the option may run a stand-alone
    add in the split format: tests/test_ffi_host.py pins that), so the twin with the three fusions off cannot be built at these
    precisions.  What is checked instead: that refusal stands; the plan with the option is, launch for launch, the plan with the two
    fusions that CAN be switched off (fuse_pointwise, stem2_kernel), except that every shortcut has its own add launch behind its
    conv and that conv carries no residual; the packed image is the same."""
    lib = _ffi.lib()
    h = plan(text, res, 4, precision)
    assert lib.rtod_plan_set_option(h, b"fuse_shortcut", 0) == -3 and "add" in _ffi.last_error()
    lib.rtod_plan_destroy(h)
    on, two = plan(text, res, 4, precision, OPT), plan(text, res, 4, precision, OFF3[1:])
    shortcuts = [L["index"] for L in describe(on)["layers"] if L["type"] == "shortcut"]
    a, b = _launches(on), _launches(two)
    assert [li.layer for li in a if li.kind == 3] == shortcuts and not any(li.kind == 3 for li in b)
    assert not any(li.fused_pointwise or li.fused_residual for li in a) and sum(li.fused_residual for li in b) == len(shortcuts)
    rest = [li for li in a if li.kind != 3]
    assert len(rest) == len(b)
    for x, y in zip(rest, b):
        assert (x.layer, x.kind, x.ksize, x.stride, x.cin, x.cout, x.fused_decode, x.fused_pointwise, x.flops_per_frame, x.weight_bytes) == \
               (y.layer, y.kind, y.ksize, y.stride, y.cin, y.cout, y.fused_decode, y.fused_pointwise, y.flops_per_frame, y.weight_bytes)
    L1 = describe(on)["layers"]
    assert all(L["fused_into"] < 0 or L1[L["fused_into"]]["type"] == "yolo" for L in L1)
    w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    assert np.array_equal(pack(on, w), pack(two, w))
    for h in (on, two):
        lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("net,precision", [("mini", 0), ("mini", 1), ("mini", 2), ("yolov3", 1), ("tiny", 0)])
def test_the_option_is_the_plan_with_the_three_fusions_off_plus_liveness(net, precision):
    text, res = {"mini": (cfgs.mini_cfg(64, 64), 64), "yolov3": (cfgs.yolov3_cfg(416, 416), 416), "tiny": (cfgs.yolov3_tiny_cfg(416, 416), 416)}[net]
    lib = _ffi.lib()
    if precision:
        _split_plan_holds_the_fusions(text, res, precision)
        return
    on, twin = plan(text, res, 4, precision, OPT), plan(text, res, 4, precision, OFF3)
    d1, d0 = describe(on), describe(twin)
    assert d1["layers"] == d0["layers"] and d1["n_launches"] == d0["n_launches"] and d1["arena_floats"] >= d0["arena_floats"]
    li0, li1 = _ffi.LaunchInfo(), _ffi.LaunchInfo()
    for k in range(d0["n_launches"]):
        assert lib.rtod_plan_get_launch(twin, k, C.byref(li0)) == 0 and lib.rtod_plan_get_launch(on, k, C.byref(li1)) == 0
        assert bytes(li0) == bytes(li1), k
    w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    assert np.array_equal(pack(on, w), pack(twin, w))
    # every buffer a trainable conv reads or writes lives to the end of the forward; no conv is fused into a shortcut
    L1, n_layers = d1["layers"], len(d1["layers"])
    convs = [c for c, _ in trainable_layers(on)]
    assert convs and all(L1[c]["fused_into"] < 0 for c in convs)
    for c in convs:
        for layer in (c - 1, c):
            buf = L1[_resolve(L1, layer)]["buf"]
            assert buf >= 0 and d1["bufs"][buf]["last"] >= n_layers - 1, (c, layer)
    # setting it and taking it back gives the default plan's description again
    back, default = plan(text, res, 4, precision, OPT + [("keep_backbone_activations", 0)]), plan(text, res, 4, precision)
    assert describe(back) == describe(default)
    for h in (on, twin, back, default):
        lib.rtod_plan_destroy(h)


def SGD(lr=1e-3):
    return _ffi.OptStep(0, lr, 0, 0, 0, 0)


def test_folded_entries_accept_every_trainable_conv_with_the_option():
    lib, err = _ffi.lib(), _ffi.last_error
    step = lambda h, layer: lib.rtod_plan_step_conv_folded(h, layer, C.byref(SGD()), ONE, ONE, None, None, None)
    upd = lambda h, layer: lib.rtod_plan_update_conv_weight(h, layer, ONE)
    scale = lambda h, layer, ch: lib.rtod_plan_conv_scale(h, layer, None, None, ch)
    text = cfgs.mini_cfg(64, 64)
    cout = {L.index: L.cout for L in build_ir(parse_cfg_text(text), 64).layers}
    for precision in (0, 1):
        on, neck = plan(text, 64, 4, precision, OPT), plan(text, 64, 4, precision, [("keep_neck_activations", 1)])
        for layer in TRAINABLE["mini"]:                               # accepted: the calls get as far as the state check
            assert step(on, layer) == -4 and "load_weights" in err(), layer
            assert upd(on, layer) == -4 and scale(on, layer, cout[layer]) == -4, layer
        for call in (lambda layer: step(on, layer), lambda layer: upd(on, layer), lambda layer: scale(on, layer, 1)):
            assert call(0) == -1 and "stem" in err()
            assert call(14) == -1 and "no BatchNorm" in err()
            assert call(4) == -1 and "not a convolution" in err()
        for layer in MINI_S2:                                         # the neck option alone keeps refusing a stride-2 conv, with the reason
            assert step(neck, layer) == -1 and "not a neck conv" in err()
        lib.rtod_plan_destroy(on)
        lib.rtod_plan_destroy(neck)
    h = plan(cfgs.yolov3_tiny_cfg(416, 416), 416, 4, 0, OPT)          # a shape-ok conv that a max-pool reads
    assert step(h, 8) == -1 and "not a trainable conv" in err() and "outside the trainable graph" in err()
    lib.rtod_plan_destroy(h)


# ---------------------------------------------------------------------------------------------- 3. the references against autograd
@pytest.mark.parametrize("shape", S2_SHAPES)
def test_the_numpy_references_are_float64_autograd_on_small_integers(shape):
    B, cout, cin, H, W = shape
    Ho, Wo = out_hw(H, W)
    rng = np.random.default_rng(B * 1000 + H * W)
    w, x, dz = rng.integers(-4, 5, (cout, cin, 3, 3)), rng.integers(-4, 5, (B, cin, H, W)), rng.integers(-4, 5, (B, cout, Ho, Wo))
    wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    out = fn.conv2d(xt, wt, stride=2, padding=1)
    assert tuple(out.shape) == (B, cout, Ho, Wo)
    out.backward(torch.from_numpy(dz.astype(np.float64)))
    assert np.array_equal(conv_dgrad_s2_ref(w, dz, H, W, np.int64).astype(np.float64), xt.grad.numpy()), shape
    assert np.array_equal(conv_wgrad_s2_ref(dz, x, np.int64).astype(np.float64), wt.grad.numpy()), shape


# ---------------------------------------------------------------------------------------------- 4. workspace sizes and refusals
@pytest.mark.parametrize("shape", S2_SHAPES + [(8, 64, 32, 208, 208), (8, 1024, 512, 26, 26), (2, 128, 64, 104, 104)])
def test_wgrad_s2_workspace_follows_the_slice_rule(shape):
    B, cout, cin, H, W = shape
    Ho, Wo = out_hw(H, W)
    S, _, _ = conv_wgrad_slices(B * Ho * Wo, cout, cin * 9)
    nb = C.c_size_t()
    assert _ffi.lib().rtod_conv_wgrad_s2_workspace(B, cout, cin, H, W, 3, C.byref(nb)) == 0
    assert nb.value == 4 * S * (cout * cin * 9 + cout), (shape, S)


def test_s2_entries_refuse_what_they_do_not_take():
    lib = _ffi.lib()
    nb = C.c_size_t()
    dgrad = lambda w=ONE, s=None, dz=ONE, y=ONE, slope=0.1, shape=(1, 1, 32, 1, 1, 3), dx=ONE: lib.rtod_conv_dgrad_s2(w, s, dz, y, slope, *shape, dx, None)
    for kw in (dict(w=None), dict(dz=None), dict(dx=None), dict(slope=float("nan")), dict(shape=(1, 1, 16, 1, 1, 3)), dict(shape=(1, 1, 48, 1, 1, 3)),
               dict(shape=(1, 1, 32, 1, 1, 1)), dict(shape=(1, 1, 32, 1, 1, 2)), dict(shape=(0, 1, 32, 1, 1, 3)), dict(shape=(1, 0, 32, 1, 1, 3)),
               dict(shape=(1, 1, 32, 0, 1, 3)), dict(shape=(1, 1, 32, 1, 0, 3)), dict(shape=(1 << 8, 1, 32, 1 << 12, 1 << 12, 3)),
               dict(shape=(1, 1 << 14, 1 << 14, 1, 1, 3))):
        assert dgrad(**kw) == -1, kw
        assert "conv_dgrad_s2" in _ffi.last_error(), kw
    wgrad = lambda dz=ONE, x=ONE, shape=(1, 1, 32, 1, 1, 3), dw=ONE, ws=ONE, nbytes=1 << 30: lib.rtod_conv_wgrad_s2(dz, x, *shape, None, dw, None, ws, nbytes, None)
    for kw in (dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None), dict(shape=(1, 1, 16, 1, 1, 3)), dict(shape=(1, 1, 32, 1, 1, 1)),
               dict(shape=(1, 1, 32, 0, 1, 3)), dict(nbytes=8), dict(ws=C.c_void_p(68))):
        assert wgrad(**kw) == -1, kw
        assert "conv_wgrad_s2" in _ffi.last_error(), kw
    for shape in ((1, 1, 16, 1, 1, 3), (1, 1, 32, 1, 1, 1), (1, 1, 32, 1, 0, 3)):
        assert lib.rtod_conv_wgrad_s2_workspace(*shape, C.byref(nb)) == -1, shape
    assert lib.rtod_conv_wgrad_s2_workspace(1, 1, 32, 1, 1, 3, None) == -1
    ptrs = (C.c_void_p * 4)(64, 64, 64, 64)
    join = lambda p=ptrs, count=2, y=ONE, slope=0.1, n=4, out=ONE: lib.rtod_grad_join(p, count, y, slope, n, out, None)
    for kw in (dict(p=None), dict(out=None), dict(count=0), dict(count=5), dict(n=0), dict(slope=float("nan")), dict(p=(C.c_void_p * 4)(64, None, 64, 64))):
        assert join(**kw) == -1, kw
        assert "grad_join" in _ffi.last_error(), kw


def test_trainer_asks_for_the_backbone_options():
    stub = lambda opts: types.SimpleNamespace(blocks=parse_cfg_text(cfgs.mini_cfg(64, 64)), net_info={"height": 64}, input_width=None, options=opts)
    assert DarknetTrainer(stub({}), trainable="backbone").trainable == "backbone"
    for opts in ({}, {"keep_head_inputs": 1}, {"keep_backbone_activations": 1}, {"keep_head_inputs": 1, "keep_neck_activations": 1}):
        t = DarknetTrainer(stub(opts), trainable="backbone")
        for call in (t.backbone_gradients, t.gradients, lambda x, b: DarknetTrainer(stub(opts)).gradients(x, b, scope="backbone")):
            with pytest.raises(RuntimeError, match="keep_backbone_activations"):
                call(None, [])
