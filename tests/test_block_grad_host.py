"""Host tests of the detection-block training path (the BatchNorm conv in front of each head conv, BatchNorm frozen):
rtod_plan_head_blocks on the shipped and the test cfgs, the liveness that option keep_block_inputs adds and nothing else, the
refusals of rtod_plan_update_conv_weight / rtod_plan_step_conv_folded / rtod_plan_conv_scale (all decided on the host), and the
argument checks and the slice rule of rtod_conv_wgrad / rtod_conv1x1_dgrad.  The device is covered by tests/test_block_grad_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest

from block_grad_cases import WGRAD_SHAPES, conv_wgrad_slices, head_blocks
from head_grad_cases import describe, pack, plan
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer

F = np.float32
ONE = C.c_void_p(64)                                                  # never dereferenced: every refusal is decided on the host


# ---------------------------------------------------------------------------------------------- rtod_plan_head_blocks
def test_head_blocks_of_the_shipped_and_the_test_cfgs(tmp_path):
    lib = _ffi.lib()
    v3, tiny, mini = cfgs.yolov3_cfg(416, 416), cfgs.yolov3_tiny_cfg(416, 416), cfgs.mini_cfg(64, 64)
    for text, res, precision, options, want in (
            (v3, 416, 0, (), [(81, 80, 79), (93, 92, 91), (105, 104, 103)]),
            (v3, 416, 1, (), [(81, 80, 79), (93, 92, 91), (105, 104, 103)]),
            (v3, 416, 1, (("k_slices_split", 1),), [(81, 80, 79), (93, 92, 91), (105, 104, 103)]),   # sliced convs pack by the generic formula
            (tiny, 416, 0, (), [(15, 14, 13), (22, 21, 20)]),
            (tiny, 416, 1, (("narrow_cin", 1),), [(15, 14, 13), (22, 21, 20)]),
            (mini, 64, 0, (), [(14, 13, 12), (22, 21, 20)]),
            (mini, 64, 2, (), [(14, 13, 12), (22, 21, 20)]),
            (cfgs.mini_fallback_cfg(64, 64), 64, 0, (), [(12, -1, -1), (16, -1, -1)]),           # a max-pool, a stride-2 conv
            (cfgs.v5_style_mini_cfg(128, 128), 128, 0, (), [(12, -1, -1), (20, -1, -1)]),        # SiLU convs
            (cfgs.stem_pool_mini_cfg(64, 64), 64, 0, (), [(4, -1, -1)]),                         # a stride-2 conv again
            (mini, 64, 0, (("bn_batch_stats", 1),), [(14, -1, -1), (22, -1, -1)]),               # the conv is not folded there
            (mini, 64, 1, (("bn_batch_stats", 1), ("bn_batch_split", 1)), [(14, -1, -1), (22, -1, -1)])):
        h = plan(text, res, 4, precision, options)
        assert head_blocks(h) == want, (res, precision, options)
        d = describe(h)
        for head, block, inp in want:
            if block >= 0:
                L = d["layers"][block]
                assert L["type"] == "convolutional" and L["bn"] and L["size"] in (1, 3) and L["stride"] == 1 and L["cin"] % 32 == 0 and block == head - 1
        one = [(C.c_int * 1)() for _ in range(3)]
        assert lib.rtod_plan_head_blocks(h, *one, 1) == len(want) and tuple(a[0] for a in one) == want[0]   # the count; capacity entries written
        assert lib.rtod_plan_head_blocks(h, None, None, None, 1) == -1 and lib.rtod_plan_head_blocks(None, None, None, None, 0) == -1
        lib.rtod_plan_destroy(h)
    d = describe(plan(tiny, 416))
    assert d["layers"][20]["type"] == "route" and d["layers"][20]["cout"] == 384 and d["layers"][21]["cin"] == 384   # the route-fed block
    # a conv without BatchNorm in front of a head is no block
    a, old, b = cfgs.stem_pool_mini_cfg(64, 64).rpartition("[convolutional]\nbatch_normalize=1\nfilters=32\nsize=3\nstride=2")
    assert old
    h = plan(a + "[convolutional]\nfilters=32\nsize=3\nstride=1" + b, 64)
    assert head_blocks(h) == [(4, -1, -1)] and not describe(h)["layers"][3]["bn"]
    lib.rtod_plan_destroy(h)


# ---------------------------------------------------------------------------------------------- keep_block_inputs: liveness only
def _resolve(layers, i):
    while layers[i]["alias_of"] >= 0:
        i = layers[i]["alias_of"]
    return i


@pytest.mark.parametrize("net,precision", [("yolov3", 0), ("yolov3", 1), ("yolov3", 2), ("tiny", 0), ("mini", 0), ("mini", 1), ("mini", 2), ("fallback", 0)])
def test_keep_block_inputs_keeps_the_block_inputs_alive_and_nothing_else(net, precision):
    text, res = {"yolov3": (cfgs.yolov3_cfg(416, 416), 416), "tiny": (cfgs.yolov3_tiny_cfg(416, 416), 416), "mini": (cfgs.mini_cfg(64, 64), 64),
                 "fallback": (cfgs.mini_fallback_cfg(64, 64), 64)}[net]
    B = 4
    off, on = plan(text, res, B, precision), plan(text, res, B, precision, [("keep_block_inputs", 1)])
    d0, d1 = describe(off), describe(on)
    n_layers = len(d1["layers"])
    assert head_blocks(off) == head_blocks(on)
    blocks = [(b, i) for _, b, i in head_blocks(on) if b >= 0]
    assert len(blocks) == {"yolov3": 3, "tiny": 2, "mini": 2, "fallback": 0}[net]
    kept = {d1["layers"][_resolve(d1["layers"], inp)]["buf"] for _, inp in blocks}
    assert len(kept) == len(blocks) and -1 not in kept
    if net == "tiny":                                                  # the second block reads route(-1, 8): its concat buffer is what stays
        assert d1["bufs"][d1["layers"][20]["buf"]]["C"] == 384 and d1["layers"][20]["buf"] in kept
    size = lambda b: (b["floats_per_frame"] * B + 63) // 64 * 64
    for i, a in enumerate(d1["bufs"]):
        if i in kept:
            assert a["last"] >= n_layers - 1                          # live to the end of the forward
        for j, b in enumerate(d1["bufs"]):
            if j <= i:
                continue
            live = not (a["last"] < b["first"] or b["last"] < a["first"])
            mem = not (a["offset"] + size(a) <= b["offset"] or b["offset"] + size(b) <= a["offset"])
            assert not (live and mem), (a, b)
            if mem and (i in kept) != (j in kept):                    # whatever shares a block input's space is dead before it is written
                hb, ob = (a, b) if i in kept else (b, a)
                assert ob["last"] < hb["first"], (hb, ob)
    # everything but liveness and arena placement is the plan without the option
    assert d0["layers"] == d1["layers"] and d0["n_launches"] == d1["n_launches"] and d1["arena_floats"] >= d0["arena_floats"]
    assert [(b["C"], b["H"], b["W"], b["first"]) for b in d0["bufs"]] == [(b["C"], b["H"], b["W"], b["first"]) for b in d1["bufs"]]
    assert [b["last"] for i, b in enumerate(d0["bufs"]) if i not in kept] == [b["last"] for i, b in enumerate(d1["bufs"]) if i not in kept]
    if not blocks:
        assert d0 == d1
    lib = _ffi.lib()
    li0, li1 = _ffi.LaunchInfo(), _ffi.LaunchInfo()
    for k in range(d0["n_launches"]):
        assert lib.rtod_plan_get_launch(off, k, C.byref(li0)) == 0 and lib.rtod_plan_get_launch(on, k, C.byref(li1)) == 0
        assert bytes(li0) == bytes(li1), k
    w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    assert np.array_equal(pack(off, w), pack(on, w))
    lib.rtod_plan_destroy(off)
    lib.rtod_plan_destroy(on)


# ---------------------------------------------------------------------------------------------- refusals, decided on the host
def SGD(lr=1e-3):
    return _ffi.OptStep(0, lr, 0, 0, 0, 0)


def ADAM(step=1):
    return _ffi.OptStep(1, 1e-2, 0.9, 0.999, 1e-8, step)


def _step(h, layer, opt=None, w=ONE, dw=ONE, moments=(ONE, ONE)):
    return _ffi.lib().rtod_plan_step_conv_folded(h, layer, C.byref(opt) if opt is not None else None, w, dw, *moments, None)


def test_folded_step_and_update_conv_weight_refusals():
    lib = _ffi.lib()
    err = _ffi.last_error
    upd = lambda h, layer, w=ONE: lib.rtod_plan_update_conv_weight(h, layer, w)
    scale = lambda h, layer, ch: lib.rtod_plan_conv_scale(h, layer, None, None, ch)
    h = plan(cfgs.mini_cfg(64, 64), 64, 4, 1)
    (head0, b0, _), (head1, b1, _) = head_blocks(h)
    assert (b0, b1) == (13, 21)
    assert _step(None, b0, SGD()) == -1 and upd(None, b0) == -1 and scale(None, b0, 1024) == -1
    assert _step(h, b0, None) == -1 and _step(h, b0, SGD(), w=None) == -1 and _step(h, b0, SGD(), dw=None) == -1 and "null" in err()
    assert upd(h, b0, None) == -1 and "null" in err()
    for call in (lambda layer: _step(h, layer, SGD()), lambda layer: upd(h, layer), lambda layer: scale(h, layer, 1)):
        assert call(head0) == -1 and "no BatchNorm" in err()                          # the head conv itself
        assert call(head0 + 1) == -1 and "not a convolution" in err()                 # the [yolo] layer
        assert call(-1) == -1 and call(1000) == -1
        assert call(0) == -1 and "not a detection block" in err() and "stem" in err()  # the stem
        assert call(2) == -1 and "pointwise" in err()                                 # guest of a fused-pointwise candidate pair
        assert call(1) == -1 and "pointwise" in err()                                 # ... and its host
        assert call(12) == -1 and "not a detection block" in err()                    # a BatchNorm conv that no head conv reads
        assert call(b0 - 1) == -1 and call(20) == -1
    for mom in ((None, ONE), (ONE, None), (None, None)):
        assert _step(h, b1, ADAM(), moments=mom) == -1 and "moment" in err(), mom
    assert _step(h, b1, ADAM(0)) == -1 and _step(h, b1, _ffi.OptStep(2, 1e-3, 0, 0, 0, 0)) == -1 and _step(h, b1, SGD(float("inf"))) == -1
    assert _step(h, b1, _ffi.OptStep(1, 1e-2, 1.0, 0.999, 1e-8, 1)) == -1 and _step(h, b1, _ffi.OptStep(1, 1e-2, 0.9, 0.999, -1.0, 1)) == -1
    assert scale(h, b1, 511) == -1 and "channels" in err()
    # a well-formed call before rtod_plan_load_weights is a state error
    assert _step(h, b0, SGD(), moments=(None, None)) == -4 and "load_weights" in err()
    assert _step(h, b1, ADAM()) == -4 and upd(h, b1) == -4 and "load_weights" in err() and scale(h, b1, 512) == -4
    lib.rtod_plan_destroy(h)
    # a narrow conv (Cin == 16) is refused by its shape; under batch-statistics BatchNorm nothing is a block
    h = plan(cfgs.narrow_mini_cfg(64, 64), 64, 4, 1, [("narrow_cin", 1)])
    assert _step(h, 1, SGD()) == -1 and "narrow" in err() and upd(h, 1) == -1 and "narrow" in err()
    lib.rtod_plan_destroy(h)
    h = plan(cfgs.mini_cfg(64, 64), 64, 4, 0, [("bn_batch_stats", 1)])
    assert _step(h, 13, SGD()) == -1 and "batch-statistics" in err() and upd(h, 13) == -1 and "batch-statistics" in err()
    lib.rtod_plan_destroy(h)


def test_trainer_asks_for_both_keep_options():
    stub = lambda opts: types.SimpleNamespace(blocks=parse_cfg_text(cfgs.mini_cfg(64, 64)), net_info={"height": 64}, input_width=None, options=opts)
    with pytest.raises(ValueError, match="trainable"):
        DarknetTrainer(stub({}), trainable="trunk")
    assert DarknetTrainer(stub({})).trainable == "heads"
    for opts in ({}, {"keep_head_inputs": 1}, {"keep_block_inputs": 1}):
        t = DarknetTrainer(stub(opts), trainable="blocks")
        for call in (t.block_gradients, t.gradients, lambda x, b: DarknetTrainer(stub(opts)).gradients(x, b, scope="blocks")):
            with pytest.raises(RuntimeError, match="keep_block_inputs"):
                call(np.zeros((1, 3, 64, 64), F), [None])
        with pytest.raises(RuntimeError, match="keep_head_inputs"):
            t.feed_forward_through_model(np.zeros((1, 3, 64, 64), F), [None])


# ---------------------------------------------------------------------------------------------- the kernels' argument checks, the slice rule
def test_conv_wgrad_argument_checks_and_workspace_follow_the_slice_rule():
    """The closed form of include/rtod.h, restated in block_grad_cases.conv_wgrad_slices, against the workspace the library asks for;
    the three YOLOv3 blocks and the two YOLOv3-tiny blocks at 416x416, batch 8, stay below 64 MB (dW of 18.9, 4.7 and 1.2 MB with
    1, 4 and 15 slices)."""
    lib = _ffi.lib()
    nb = C.c_size_t()
    for shape in ((0, 1, 32, 1, 1, 3), (1, 0, 32, 1, 1, 3), (1, 1, 0, 1, 1, 3), (1, 1, 48, 1, 1, 3), (1, 1, 16, 1, 1, 1), (1, 1, 32, 0, 1, 3), (1, 1, 32, 1, 0, 3),
                  (1, 1, 32, 1, 1, 2), (1, 1, 32, 1, 1, 5), (1, 1, 32, 1, 1, 0), (1 << 8, 1, 32, 1 << 12, 1 << 12, 3), (1, 1 << 14, 1 << 14, 1, 1, 3)):
        assert lib.rtod_conv_wgrad_workspace(*shape, C.byref(nb)) == -1, shape
        assert lib.rtod_conv_wgrad(ONE, ONE, *shape, None, ONE, None, ONE, 1 << 30, None) == -1, shape
    assert lib.rtod_conv_wgrad_workspace(1, 1, 32, 1, 1, 3, None) == -1
    table = (((8, 1024, 512, 13, 13, 3), 1), ((8, 512, 256, 26, 26, 3), 4), ((8, 256, 128, 52, 52, 3), 15),          # YOLOv3's blocks
             ((8, 512, 256, 13, 13, 3), 4), ((8, 256, 384, 26, 26, 3), 5),                                           # YOLOv3-tiny's
             ((1, 1, 32, 1, 1, 3), 1), ((2, 18, 32, 2, 2, 3), 1), ((3, 255, 96, 13, 13, 3), 16), ((3, 255, 96, 13, 13, 1), 16),
             ((1, 64, 64, 5, 7, 3), 5), ((2, 40, 32, 4, 6, 3), 6), ((1, 64, 256, 4, 4, 3), 2), ((1, 64, 512, 3, 3, 3), 2),
             ((1, 64, 64, 16, 8, 3), 16), ((1, 64, 64, 127, 1, 3), 16), ((1, 64, 64, 128, 1, 1), 16), ((2, 64, 1024, 2, 2, 1), 1))
    for (B, cout, cin, H, W, size), slices in table:
        K, ncol = B * H * W, cin * size * size
        S, L, cap = conv_wgrad_slices(K, cout, ncol)
        assert S == slices and L % 8 == 0 and (S - 1) * L < K <= S * L and S <= cap <= 16, (B, cout, cin, H, W, size, S, L, cap)
        assert lib.rtod_conv_wgrad_workspace(B, cout, cin, H, W, size, C.byref(nb)) == 0
        assert nb.value == 4 * S * (cout * ncol + cout) and nb.value <= 64 << 20, (B, cout, cin, H, W, size)
        for kw in (dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None), dict(ws=C.c_void_p(68)), dict(nbytes=nb.value - 1)):
            a = dict(dz=ONE, x=ONE, dw=ONE, ws=ONE, nbytes=nb.value)
            a.update(kw)
            assert lib.rtod_conv_wgrad(a["dz"], a["x"], B, cout, cin, H, W, size, None, a["dw"], None, a["ws"], a["nbytes"], None) == -1, kw
            assert "conv_wgrad" in _ffi.last_error()
    # the rule sees K and the tile count alone: a grid of a thousand tiles is never sliced, a single tile gets the 1x1 rule's 16
    assert conv_wgrad_slices(10 ** 6, 1024, 4608)[0] == 1 and conv_wgrad_slices(10 ** 6, 64, 64)[0] == 16 and conv_wgrad_slices(7, 64, 64)[0] == 1


def test_wgrad_shapes_span_the_slice_rule():
    """The shapes of the GPU tests against the slice counts the LIBRARY reports (workspace bytes / (4 (Cout ncol + Cout))), 3x3."""
    lib = _ffi.lib()
    nb = C.c_size_t()
    S = {}
    for B, cout, cin, H, W in WGRAD_SHAPES:
        assert lib.rtod_conv_wgrad_workspace(B, cout, cin, H, W, 3, C.byref(nb)) == 0
        S[(B, cout, cin, H, W)], rest = divmod(nb.value, 4 * (cout * cin * 9 + cout))
        assert rest == 0 and S[(B, cout, cin, H, W)] == conv_wgrad_slices(B * H * W, cout, cin * 9)[0]
    assert S[(1, 64, 512, 2, 4)] == 1 and S[(1, 1, 32, 1, 1)] == 1
    assert S[(2, 256, 928, 4, 4)] == 2 == conv_wgrad_slices(32, 256, 928 * 9)[2]               # the tile count caps the slices
    assert S[(1, 64, 64, 16, 8)] == S[(1, 64, 64, 127, 1)] == S[(3, 255, 96, 13, 13)] == 16    # K = 128 on a slice boundary (16 x 8), 127 one short
    assert conv_wgrad_slices(128, 64, 576)[1] == conv_wgrad_slices(127, 64, 576)[1] == 8 and conv_wgrad_slices(48, 40, 288)[1] % 32 != 0


def test_conv1x1_dgrad_argument_checks():
    lib = _ffi.lib()
    call = lambda w=ONE, dz=ONE, y=ONE, slope=0.1, shape=(1, 1, 32, 1), dx=ONE: lib.rtod_conv1x1_dgrad(w, dz, y, slope, *shape, dx, None)
    for kw in (dict(w=None), dict(dz=None), dict(dx=None), dict(slope=float("nan")), dict(shape=(0, 1, 32, 1)), dict(shape=(1, 0, 32, 1)), dict(shape=(1, 1, 0, 1)),
               dict(shape=(1, 1, 48, 1)), dict(shape=(1, 1, 16, 1)), dict(shape=(1, 1, 32, 0)), dict(shape=(1 << 16, 1, 32, 1 << 16))):
        assert call(**kw) == -1, kw
        assert "conv1x1_dgrad" in _ffi.last_error(), kw
