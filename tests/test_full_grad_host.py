"""Host tests of the "full" training scope (BatchNorm frozen): rtod_plan_full_layers on YOLOv3-tiny, pool_train_mini_cfg and YOLOv3,
rtod_plan_trainable_layers unchanged beside it, what option keep_full_activations keeps, the numpy reference of the max-pool backward
against CPU autograd of the reference's two modules, the slice rule of rtod_conv_wgrad_thin, every refusal of the three new entries and
of the folded-conv entries under the new scope, and the trainer's errors — all decided on the host.  The device is covered by
tests/test_full_grad_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from backbone_grad_cases import TRAINABLE, trainable_layers
from full_grad_cases import POOL_MINI_FULL, POOL_MINI_TRAINABLE, POOL_SHAPES, TINY_FULL, full_layers, maxpool_grad_ref, pool_out_hw, torch_pool_grad
from head_grad_cases import describe, plan
from realtimeobjectdetection_amd import _ffi, cfgs
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer

F = np.float32
ONE = C.c_void_p(64)                                                  # never dereferenced: every refusal is decided on the host
OPT = [("keep_full_activations", 1)]
BACKBONE = [("keep_backbone_activations", 1)]


# ---------------------------------------------------------------------------------------------- 1. rtod_plan_full_layers
def test_full_layers_on_tiny():
    lib = _ffi.lib()
    text = cfgs.yolov3_tiny_cfg(416, 416)
    h = plan(text, 416, 4, 0, OPT)
    got = full_layers(h)
    assert [c for c, _ in got] == TINY_FULL and all(i == c - 1 for c, i in got) and got[0] == (0, -1)
    assert [c for c, _ in trainable_layers(h)] == TRAINABLE["tiny"]
    one = [(C.c_int * 1)() for _ in range(2)]
    assert lib.rtod_plan_full_layers(h, *one, 1) == len(got) and (one[0][0], one[1][0]) == got[0]
    assert lib.rtod_plan_full_layers(h, None, None, 1) == -1 and lib.rtod_plan_full_layers(None, None, None, 0) == -1
    lib.rtod_plan_destroy(h)
    for opts in ([], BACKBONE):                                       # the listing does not need the option on tiny; the trainable one does not move
        h = plan(text, 416, 4, 0, opts)
        assert [c for c, _ in full_layers(h)] == TINY_FULL and [c for c, _ in trainable_layers(h)] == TRAINABLE["tiny"]
        lib.rtod_plan_destroy(h)
    # split-f16: layer 0 runs an fp32 stem into the split format and layer 2 is packed narrow: neither is a member, the pools are walked
    h = plan(text, 416, 4, 1, [("narrow_cin", 1)] + OPT)
    assert [c for c, _ in full_layers(h)] == TINY_FULL[2:] and [c for c, _ in trainable_layers(h)] == TRAINABLE["tiny"]
    lib.rtod_plan_destroy(h)
    h = plan(text, 416, 4, 0, [("bn_batch_stats", 1)] + OPT)          # nothing is folded, nothing is trainable
    assert full_layers(h) == []
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("height,width", [(64, 64), (64, 96), (40, 40)])
def test_full_layers_on_pool_train_mini(height, width):
    lib = _ffi.lib()
    for stem, precision in ((16, 0), (32, 0), (32, 1)):
        text = cfgs.pool_train_mini_cfg(height, width, stem=stem)
        h = lib_plan(text, height, width, precision, OPT)
        assert [c for c, _ in full_layers(h)] == POOL_MINI_FULL[stem], (stem, precision)
        assert [c for c, _ in trainable_layers(h)] == POOL_MINI_TRAINABLE
        lib.rtod_plan_destroy(h)
        h = lib_plan(text, height, width, precision, BACKBONE)
        assert [c for c, _ in trainable_layers(h)] == POOL_MINI_TRAINABLE
        lib.rtod_plan_destroy(h)
    h = lib_plan(cfgs.pool_train_mini_cfg(height, width, stem=32), height, width, 0, OPT + [("stem_kernel", 0)])
    assert [c for c, _ in full_layers(h)] == POOL_MINI_FULL[16]       # layer 0 on the generic layout: a member
    lib.rtod_plan_destroy(h)


def lib_plan(text, height, width, precision, options):
    """head_grad_cases.plan for a rectangular input."""
    lib = _ffi.lib()
    h = C.c_void_p()
    raw = text.encode()
    assert lib.rtod_plan_create_rect(raw, len(raw), height, width, 4, 0, C.byref(h)) == 0, _ffi.last_error()
    for name, value in options:
        assert lib.rtod_plan_set_option(h, name.encode(), value) == 0, _ffi.last_error()
    if precision:
        assert lib.rtod_plan_set_precision(h, precision) == 0, _ffi.last_error()
    return h


def test_full_layers_on_yolov3():
    lib = _ffi.lib()
    text = cfgs.yolov3_cfg(416, 416)
    ir = build_ir(parse_cfg_text(text), 416)
    convs = [L.index for L in ir.layers if L.type == "convolutional" and L.bn]
    assert len(convs) == 72
    h = plan(text, 416, 2, 0, OPT)                                    # layer 0 runs the stem kernel: the full graph is the trainable graph
    assert [c for c, _ in full_layers(h)] == [c for c, _ in trainable_layers(h)] == convs[1:]
    lib.rtod_plan_destroy(h)
    h = plan(text, 416, 2, 0, OPT + [("stem_kernel", 0)])
    assert [c for c, _ in full_layers(h)] == convs and [c for c, _ in trainable_layers(h)] == convs[1:]
    lib.rtod_plan_destroy(h)
    h = plan(text, 416, 2, 0, BACKBONE)
    assert [c for c, _ in trainable_layers(h)] == convs[1:]
    lib.rtod_plan_destroy(h)


# ---------------------------------------------------------------------------------------------- 2. the option
def _resolve(layers, i):
    while layers[i]["alias_of"] >= 0:
        i = layers[i]["alias_of"]
    return i


def test_the_option_holds_the_fusions_and_keeps_every_full_graph_buffer():
    lib = _ffi.lib()
    text = cfgs.yolov3_tiny_cfg(416, 416)
    on, twin, default = plan(text, 416, 4, 0, OPT), plan(text, 416, 4, 0, BACKBONE), plan(text, 416, 4, 0)
    d1, d0 = describe(on), describe(twin)
    assert d1["layers"] == d0["layers"] and d1["n_launches"] == d0["n_launches"] and d1["arena_floats"] >= d0["arena_floats"]
    L1, n_layers = d1["layers"], len(d1["layers"])
    pools = [L["index"] for L in L1 if L["type"] == "maxpool"]
    assert len(pools) == 6
    for layer in TINY_FULL[1:] + [c - 1 for c in TINY_FULL[1:]] + pools:      # what a full-graph conv or pool reads or writes lives to the end
        buf = L1[_resolve(L1, layer)]["buf"]
        assert buf >= 0 and d1["bufs"][buf]["last"] >= n_layers - 1, layer
    back = plan(text, 416, 4, 0, OPT + [("keep_full_activations", 0)])
    assert describe(back) == describe(default)
    for h in (on, twin, default, back):
        lib.rtod_plan_destroy(h)
    # mini_cfg has shortcuts: the option holds the three fusions as keep_backbone_activations does
    text = cfgs.mini_cfg(64, 64)
    on, twin = plan(text, 64, 4, 0, OPT), plan(text, 64, 4, 0, BACKBONE)
    assert describe(on)["layers"] == describe(twin)["layers"] and [c for c, _ in full_layers(on)] == TRAINABLE["mini"]
    lib.rtod_plan_destroy(on)
    lib.rtod_plan_destroy(twin)


def SGD(lr=1e-3):
    return _ffi.OptStep(0, lr, 0, 0, 0, 0)


def test_folded_entries_accept_every_full_graph_conv_and_refuse_the_rest():
    lib, err = _ffi.lib(), _ffi.last_error
    step = lambda h, layer: lib.rtod_plan_step_conv_folded(h, layer, C.byref(SGD()), ONE, ONE, None, None, None)
    upd = lambda h, layer: lib.rtod_plan_update_conv_weight(h, layer, ONE)
    scale = lambda h, layer, ch: lib.rtod_plan_conv_scale(h, layer, None, None, ch)
    text = cfgs.yolov3_tiny_cfg(416, 416)
    cout = {L.index: L.cout for L in build_ir(parse_cfg_text(text), 416).layers}
    on = plan(text, 416, 4, 0, OPT)
    for layer in TINY_FULL:                                           # accepted: the calls get as far as the state check
        assert step(on, layer) == -4 and "load_weights" in err(), layer
        assert upd(on, layer) == -4 and scale(on, layer, cout[layer]) == -4, layer
    for call in (lambda layer: step(on, layer), lambda layer: upd(on, layer), lambda layer: scale(on, layer, 1)):
        assert call(15) == -1 and "no BatchNorm" in err()
        assert call(1) == -1 and "not a convolution" in err()
    lib.rtod_plan_destroy(on)
    bb = plan(text, 416, 4, 0, BACKBONE)                              # the backbone option keeps refusing what a max-pool reads, and layer 0
    assert step(bb, 8) == -1 and "not a trainable conv" in err() and step(bb, 0) == -1 and "not a trainable conv" in err()
    lib.rtod_plan_destroy(bb)
    # a narrow-layout conv and a split plan's layer 0 stay refused under the new scope, with the existing texts
    sp = plan(text, 416, 4, 1, [("narrow_cin", 1)] + OPT)
    assert step(sp, 2) == -1 and "not a full-graph conv" in err() and "narrow" in err()
    assert step(sp, 0) == -1 and "not a full-graph conv" in err()
    lib.rtod_plan_destroy(sp)
    v3 = plan(cfgs.yolov3_cfg(416, 416), 416, 2, 0, OPT)              # a stem-layout layer 0
    assert step(v3, 0) == -1 and "not a full-graph conv" in err() and "stem" in err()
    lib.rtod_plan_destroy(v3)


def test_a_symmetric_pool_is_not_traversable():
    """A size-5 / stride-1 symmetric pool (the SPPF extension) has no backward entry: it and everything that only it connects to the loss
    stay outside the full graph."""
    lib = _ffi.lib()
    nout = 3 * 8
    L = cfgs._net(64, 64) + cfgs._conv(32, 3, 1) + cfgs._maxpool(2, 2) + cfgs._conv(32, 3, 1)
    L += ["[maxpool]", "size=5", "stride=1", "symmetric=1", ""] + cfgs._conv(32, 3, 1) + cfgs._maxpool(2, 2)
    L += cfgs._conv(nout, 1, 1, bn=False, act="linear") + cfgs._yolo((0, 1, 2), cfgs._ANCHORS_V3, 9, 3)
    h = plan("\n".join(L) + "\n", 64, 2, 0, OPT + [("stem_kernel", 0)])
    assert [c for c, _ in full_layers(h)] == [4]                      # behind the symmetric pool (layer 3) alone
    lib.rtod_plan_destroy(h)


# ---------------------------------------------------------------------------------------------- 3. the reference against autograd
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_the_numpy_pool_backward_is_autograd_of_the_two_modules_on_ties(shape):
    B, C_, H, W, stride = shape
    Ho, Wo = pool_out_hw(H, W, stride)
    rng = np.random.default_rng(B * 1000 + H * W + stride)
    x, dz = rng.integers(0, 3, (B, C_, H, W)).astype(F), rng.integers(0, 3, (B, C_, Ho, Wo)).astype(F)
    want = torch_pool_grad(dz, x, stride)
    got, mass = maxpool_grad_ref(dz, x, stride, np.float64)
    assert np.array_equal(got, want.astype(np.float64)) and np.array_equal(mass, got), shape       # dz >= 0: the mass is the sum
    if stride == 2:
        assert not got[:, :, 2 * Ho:, :].any() and not got[:, :, :, 2 * Wo:].any()


# ---------------------------------------------------------------------------------------------- 4. the slice rule, workspaces, refusals
def _slices(shape):
    s, n = C.c_int(), C.c_int()
    assert _ffi.lib().rtod_conv_wgrad_thin_slices(*shape, C.byref(s), C.byref(n)) == 0, _ffi.last_error()
    return s.value, n.value


def test_thin_slices_fill_the_device_and_keep_every_chain_inside_the_limit():
    LIMIT = 1024                                                      # rtod.h: the longest chain measured inside the 4 x gate
    S, L = _slices((8, 16, 3, 416, 416, 3))                           # tiny's layer 0 at 416 x 416, batch 8: one 32 x 128 tile
    K = 8 * 416 * 416
    assert S * 1 >= 1024 and L <= LIMIT and (S - 1) * L < K <= S * L
    S2, L2 = _slices((8, 32, 16, 208, 208, 3))                        # layer 2: 32 x 144, two tiles
    assert S2 * 2 >= 1000 and L2 <= LIMIT and (S2 - 1) * L2 < 8 * 208 * 208 <= S2 * L2
    for shape in ((1, 1, 1, 1, 1, 3), (2, 16, 3, 63, 65, 3), (1, 70, 5, 9, 9, 3), (64, 16, 3, 1024, 1024, 3)):
        S, L = _slices(shape)
        K = shape[0] * shape[3] * shape[4]
        assert 256 <= L <= LIMIT and L % 8 == 0 and (S - 1) * L < K <= S * L, shape
        nb = C.c_size_t()
        assert _ffi.lib().rtod_conv_wgrad_thin_workspace(*shape, C.byref(nb)) == 0 and nb.value == 4 * S * shape[1] * shape[2] * shape[5] ** 2
    assert _slices((2, 16, 3, 63, 65, 3)) == (32, 256)                # 8190 = 31 * 256 + 254


def test_the_new_entries_refuse_what_they_do_not_take():
    lib, err = _ffi.lib(), _ffi.last_error
    nan = float("nan")
    pool = lambda dz=ONE, x=ONE, slope=0.1, shape=(1, 1, 4, 4), size=2, stride=2, dx=ONE: lib.rtod_maxpool_grad(dz, x, slope, *shape, size, stride, dx, None)
    for kw in (dict(dz=None), dict(x=None), dict(dx=None), dict(size=5, stride=1), dict(size=3), dict(size=1), dict(stride=3), dict(stride=0), dict(slope=nan),
               dict(shape=(0, 1, 4, 4)), dict(shape=(1, 0, 4, 4)), dict(shape=(1, 1, 0, 4)), dict(shape=(1, 1, 4, 0)), dict(shape=(1, 1, 1 << 16, 1 << 16))):
        assert pool(**kw) == -1, kw
        assert "maxpool_grad" in err(), kw
    wgrad = lambda dz=ONE, x=ONE, shape=(1, 1, 3, 1, 1, 3), dw=ONE, ws=ONE, nbytes=1 << 30: lib.rtod_conv_wgrad_thin(dz, x, *shape, None, dw, ws, nbytes, None)
    for kw in (dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None), dict(shape=(1, 1, 0, 1, 1, 3)), dict(shape=(1, 1, 3, 1, 1, 2)), dict(shape=(1, 1, 3, 1, 1, 5)),
               dict(shape=(0, 1, 3, 1, 1, 3)), dict(shape=(1, 0, 3, 1, 1, 3)), dict(shape=(1, 1, 3, 0, 1, 3)), dict(shape=(1, 1, 3, 1, 0, 3)),
               dict(shape=(1 << 8, 1, 3, 1 << 12, 1 << 12, 3)), dict(shape=(1, 1 << 14, 1 << 14, 1, 1, 3)), dict(nbytes=8), dict(ws=C.c_void_p(68))):
        assert wgrad(**kw) == -1, kw
        assert "conv_wgrad_thin" in err(), kw
    nb, s = C.c_size_t(), C.c_int()
    for shape in ((1, 1, 0, 1, 1, 3), (1, 1, 3, 1, 1, 2), (1, 1, 3, 1, 0, 3), (1 << 8, 1, 3, 1 << 12, 1 << 12, 3)):
        assert lib.rtod_conv_wgrad_thin_workspace(*shape, C.byref(nb)) == -1, shape
        assert lib.rtod_conv_wgrad_thin_slices(*shape, C.byref(s), C.byref(s)) == -1, shape
    assert lib.rtod_conv_wgrad_thin_workspace(1, 1, 3, 1, 1, 3, None) == -1 and lib.rtod_conv_wgrad_thin_slices(1, 1, 3, 1, 1, 3, None, None) == -1
    dgrad = lambda w=ONE, sc=None, dz=ONE, y=ONE, slope=0.1, shape=(1, 1, 16, 1, 1, 3), dx=ONE: lib.rtod_conv_dgrad_thin(w, sc, dz, y, slope, *shape, dx, None)
    for kw in (dict(w=None), dict(dz=None), dict(dx=None), dict(slope=nan), dict(shape=(1, 1, 0, 1, 1, 3)), dict(shape=(1, 1, 16, 1, 1, 2)),
               dict(shape=(0, 1, 16, 1, 1, 3)), dict(shape=(1, 0, 16, 1, 1, 3)), dict(shape=(1, 1, 16, 0, 1, 3)), dict(shape=(1, 1, 16, 1, 0, 3)),
               dict(shape=(1 << 8, 1, 16, 1 << 12, 1 << 12, 3)), dict(shape=(1, 1 << 14, 1 << 14, 1, 1, 3))):
        assert dgrad(**kw) == -1, kw
        assert "conv_dgrad_thin" in err(), kw
    # the existing entries keep refusing a Cin that is no multiple of 32
    assert lib.rtod_conv_dgrad(ONE, None, ONE, ONE, 0.1, 1, 1, 16, 1, 1, 3, ONE, None) == -1 and "multiple of 32" in err()
    assert lib.rtod_conv_wgrad(ONE, ONE, 1, 1, 16, 1, 1, 3, None, ONE, None, ONE, 1 << 30, None) == -1 and "multiple of 32" in err()


def test_trainer_asks_for_the_full_options():
    stub = lambda opts: types.SimpleNamespace(blocks=parse_cfg_text(cfgs.pool_train_mini_cfg(64, 64)), net_info={"height": 64}, input_width=None, options=opts)
    assert DarknetTrainer(stub({}), trainable="full").trainable == "full" and "full" in DarknetTrainer.SCOPES
    for opts in ({}, {"keep_head_inputs": 1}, {"keep_full_activations": 1}, {"keep_head_inputs": 1, "keep_backbone_activations": 1}):
        t = DarknetTrainer(stub(opts), trainable="full")
        for call in (t.full_gradients, t.gradients, lambda x, b: DarknetTrainer(stub(opts)).gradients(x, b, scope="full")):
            with pytest.raises(RuntimeError, match="keep_full_activations"):
                call(None, [])
    with pytest.raises(ValueError, match="'full'"):
        DarknetTrainer(stub({}), trainable="everything")
