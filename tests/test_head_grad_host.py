"""Host tests of the head-gradient path: tests/head_grad_ref.py against the fixture recorded from the reference's autograd
(tests/golden/yolo_loss_grad.npz), the argument checks and workspace sizes of the new entry points (all decided on the host),
rtod_plan_head_layers, the liveness that option keep_head_inputs adds, and the per-conv pack function through
rtod_plan_pack_weights.  The device itself is covered by tests/test_head_grad_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest

import head_grad_ref as G
import loss_ref as R
from head_grad_cases import conv_stream_ranges, describe, fixture_dense, head_layers, load_grad_cases, pack, plan, wgrad_slices
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer, make_heads

F = np.float32


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_grad_cases(golden_dir)


def test_head_grad_ref_against_every_fixture_case(cases):
    assert [c["name"] for c in cases] == ["tiny_b1", "tiny_b2", "tiny_b3", "v3_b1"]
    for c in cases:
        r = G.loss_and_grads(c["raws"], c["images"], c["heads"])
        assert r["status"] == 0 and np.array_equal(np.flatnonzero(r["mask"].reshape(-1)), c["rows"]), c["name"]
        # float64 on both sides: the recorded autograd result differs from the closed form by roundings of doubles only.  The
        # targets' tw / th may sit log_ulps float32 ulps from the reference's: 2 w = 10 times that on columns 2, 3 of g and dz
        m = r["mask"]
        assert not r["g"][~m][:, :4].any() and not r["g"][~m][:, 5:].any() and np.array_equal(r["g"][~m][:, 4], r["pred"][~m][:, 4])
        for which, got in (("g", r["g"]), ("dz", r["dz"])):
            want = fixture_dense(c, which)
            if which == "g":                                          # recorded for the object rows only
                want[~m] = got[~m]
            assert np.array_equal(got == 0, want == 0), (c["name"], which)               # the zero pattern is exact
            tol = 1e-13 * np.maximum(np.abs(want), 1.0)
            tol[..., 2:4] += 10.0 * int(c["log_ulps"]) * np.spacing(np.abs(r["target"][..., 2:4]).astype(F)).astype(np.float64)
            assert (np.abs(got - want) <= tol).all(), (c["name"], which, float(np.abs(got - want).max()))
        terms = R.components(r["pred"], r["target"], r["mask"])[1]
        slack = float((10.0 * np.abs(r["pred"] - r["target"])[r["mask"]][:, 2:4] * int(c["log_ulps"]) * np.spacing(np.abs(r["target"][r["mask"]][:, 2:4]).astype(F))).sum())
        assert abs(r["components"][0] - float(c["grad_loss64"])) <= R.sum_bound(float(c["grad_loss64"]), sum(terms)) + slack, c["name"]
        # the recorded floor is what the recorded float32 gradients give against the float64 ones
        for which, raw in (("g", False), ("dz", True)):
            d = G.scale(r["pred"], r["target"], r["mask"], raw).reshape(-1, 85)[c["rows"]]
            rms, mx = G.relative_error(c["grad_%s_rows32" % which], c["grad_%s_rows64" % which], d)
            floor = c["grad_floor_" + which]
            assert 0 < floor[0] < 1e-6 and floor[0] <= floor[1] < 1e-4 and mx <= floor[1] * (1 + 1e-9), (c["name"], which, floor, rms, mx)
        # sparse: the A objectness channels everywhere plus 84 more per object row
        assert int((r["dz"] != 0).sum()) <= c["B"] * c["N"] + 84 * len(c["rows"])


def test_reshuffle_is_predict_transforms():
    raw = np.arange(2 * 3 * 7 * 2 * 5, dtype=np.float64).reshape(2, 21, 2, 5)
    rows = G.rows_from_raw(raw, 3, 7)
    assert rows.shape == (2, 30, 7)
    for b, a, c_, gy, gx in ((0, 0, 0, 0, 0), (1, 2, 6, 1, 4), (1, 1, 3, 0, 2)):
        assert rows[b, (gy * 5 + gx) * 3 + a, c_] == raw[b, a * 7 + c_, gy, gx]
    assert np.array_equal(G.raw_from_rows(rows, 3, 2, 5), raw)


# ---------------------------------------------------------------------------------------------- argument checks, workspace sizes
def _heads(n=1, grid=2, anchors=((10, 14),)):
    arr = make_heads([(grid, grid, 32, list(anchors)[:8])] * n)
    for q in arr:
        q.n_anchors = len(anchors)
    return arr


def test_yolo_loss_grad_argument_checks():
    lib = _ffi.lib()
    one = C.c_void_p(64)                                              # never dereferenced: every refusal is decided on the host
    N = 4

    def call(pred=one, batch=1, n_rows=N, num_class=1, heads=_heads(), n_heads=1, boxes=one, offs=one, min_box=4.0, grad_raw=one, status=one, ws=one, nbytes=1 << 20):
        return lib.rtod_yolo_loss_grad(pred, batch, n_rows, num_class, heads, n_heads, boxes, offs, min_box, grad_raw, None, None, None, status, ws, nbytes, None)
    for kw in (dict(pred=None), dict(boxes=None), dict(offs=None), dict(grad_raw=None), dict(status=None), dict(ws=None), dict(heads=None),
               dict(batch=0), dict(n_rows=0), dict(num_class=0), dict(n_heads=0), dict(n_heads=5), dict(n_rows=5), dict(min_box=float("nan")),
               dict(nbytes=8), dict(ws=C.c_void_p(68)), dict(heads=_heads(anchors=[(1, 1)] * 9)), dict(heads=_heads(anchors=[(0, 3)]))):
        assert call(**kw) == -1, kw
        assert "yolo_loss_grad" in _ffi.last_error(), kw
    need, need_loss = C.c_size_t(), C.c_size_t()
    assert lib.rtod_yolo_loss_workspace(3, 2535, C.byref(need_loss)) == 0                # the workspace is rtod_yolo_loss's
    assert call(batch=3, n_rows=2535, heads=make_heads([(13, 13, 32, [(1, 1)] * 3), (26, 26, 16, [(1, 1)] * 3)]), n_heads=2, nbytes=need_loss.value - 1) == -1
    assert "workspace" in _ffi.last_error()


def test_wgrad_argument_checks_and_workspace_follow_the_slice_rule():
    lib = _ffi.lib()
    one = C.c_void_p(64)
    nb = C.c_size_t()
    for shape in ((0, 1, 32, 1), (1, 0, 32, 1), (1, 1, 0, 1), (1, 1, 48, 1), (1, 1, 16, 1), (1, 1, 32, 0), (1 << 16, 1, 32, 1 << 16)):
        assert lib.rtod_conv1x1_wgrad_workspace(*shape, C.byref(nb)) == -1, shape
        assert lib.rtod_conv1x1_wgrad(one, one, *shape, one, one, one, 1 << 30, None) == -1, shape
    assert lib.rtod_conv1x1_wgrad_workspace(1, 1, 32, 1, None) == -1
    for (B, cout, cin, P), slices in (((1, 1, 32, 1), 1), ((1, 255, 32, 4), 1), ((3, 255, 96, 169), 16), ((2, 24, 64, 676), 16), ((8, 255, 1024, 4), 4),
                                      ((8, 255, 1024, 169), 16), ((8, 255, 256, 2704), 16), ((1, 7, 32, 9), 2), ((1, 7, 32, 129), 9)):
        S, L = wgrad_slices(B * P)
        assert S == slices and L % 8 == 0 and (S - 1) * L < B * P <= S * L and S <= 16, (B, P, S, L)
        assert lib.rtod_conv1x1_wgrad_workspace(B, cout, cin, P, C.byref(nb)) == 0
        assert nb.value == 4 * S * (cout * cin + cout), (B, cout, cin, P)
        for kw in (dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None), dict(ws=C.c_void_p(68)), dict(nbytes=nb.value - 1)):
            a = dict(dz=one, x=one, dw=one, ws=one, nbytes=nb.value)
            a.update(kw)
            assert lib.rtod_conv1x1_wgrad(a["dz"], a["x"], B, cout, cin, P, a["dw"], None, a["ws"], a["nbytes"], None) == -1, kw
            assert "conv1x1_wgrad" in _ffi.last_error()


# ---------------------------------------------------------------------------------------------- plan: heads, liveness, update_conv
def test_head_layers_of_yolov3_tiny_and_the_fallback_cfg(tmp_path):
    lib = _ffi.lib()
    for text, res, want in ((cfgs.yolov3_cfg(416, 416), 416, [(81, 80), (93, 92), (105, 104)]), (cfgs.yolov3_tiny_cfg(416, 416), 416, [(15, 14), (22, 21)]),
                            (cfgs.mini_fallback_cfg(64, 64), 64, [(12, 11), (16, 15)])):
        h = plan(text, res)
        assert head_layers(h) == want
        d = describe(h)
        for conv, inp in want:
            assert d["layers"][conv]["type"] == "convolutional" and not d["layers"][conv]["bn"] and d["layers"][conv + 1]["type"] == "yolo"
        conv = (C.c_int * 1)()
        inp = (C.c_int * 1)()
        assert lib.rtod_plan_head_layers(h, conv, inp, 1) == len(want) and (conv[0], inp[0]) == want[0]   # the count, capacity entries written
        assert lib.rtod_plan_head_layers(h, None, None, 1) == -1 and lib.rtod_plan_head_layers(None, None, None, 0) == -1
        lib.rtod_plan_destroy(h)
        from realtimeobjectdetection_amd.darknet import Darknet
        assert Darknet(cfgs.write_cfg(str(tmp_path / "m.cfg"), text), False).head_layers() == want


def _resolve(layers, i):
    while layers[i]["alias_of"] >= 0:
        i = layers[i]["alias_of"]
    return i


@pytest.mark.parametrize("net,precision", [("yolov3", 0), ("yolov3", 1), ("tiny", 0), ("mini", 1), ("mini", 2), ("fallback", 0)])
def test_keep_head_inputs_keeps_the_head_inputs_alive_and_nothing_else(net, precision):
    text, res = {"yolov3": (cfgs.yolov3_cfg(416, 416), 416), "tiny": (cfgs.yolov3_tiny_cfg(416, 416), 416), "mini": (cfgs.mini_cfg(64, 64), 64),
                 "fallback": (cfgs.mini_fallback_cfg(64, 64), 64)}[net]
    B = 4
    off, on = plan(text, res, B, precision), plan(text, res, B, precision, [("keep_head_inputs", 1)])
    d0, d1 = describe(off), describe(on)
    n_layers = len(d1["layers"])
    head_bufs = {d1["layers"][_resolve(d1["layers"], inp)]["buf"] for _, inp in head_layers(on)}
    assert len(head_bufs) == len(head_layers(on)) and -1 not in head_bufs
    size = lambda b: (b["floats_per_frame"] * B + 63) // 64 * 64
    for i, a in enumerate(d1["bufs"]):
        if i in head_bufs:
            assert a["last"] >= n_layers - 1                          # live to the end of the forward
        for j, b in enumerate(d1["bufs"]):
            if j <= i:
                continue
            live = not (a["last"] < b["first"] or b["last"] < a["first"])
            mem = not (a["offset"] + size(a) <= b["offset"] or b["offset"] + size(b) <= a["offset"])
            assert not (live and mem), (a, b)
            if mem and (i in head_bufs) != (j in head_bufs):          # whatever shares a head input's space is dead before it is written
                hb, ob = (a, b) if i in head_bufs else (b, a)
                assert ob["last"] < hb["first"], (hb, ob)
    # everything but liveness and arena placement is the plan without the option
    assert d0["layers"] == d1["layers"] and d0["n_launches"] == d1["n_launches"] and d1["arena_floats"] >= d0["arena_floats"]
    assert [(b["C"], b["H"], b["W"], b["first"]) for b in d0["bufs"]] == [(b["C"], b["H"], b["W"], b["first"]) for b in d1["bufs"]]
    assert [b["last"] for i, b in enumerate(d0["bufs"]) if i not in head_bufs] == [b["last"] for i, b in enumerate(d1["bufs"]) if i not in head_bufs]
    lib = _ffi.lib()
    li0, li1 = _ffi.LaunchInfo(), _ffi.LaunchInfo()
    for k in range(d0["n_launches"]):
        assert lib.rtod_plan_get_launch(off, k, C.byref(li0)) == 0 and lib.rtod_plan_get_launch(on, k, C.byref(li1)) == 0
        assert bytes(li0) == bytes(li1), k
    w = synth.synth_weights(build_ir(parse_cfg_text(text), res))
    assert np.array_equal(pack(off, w), pack(on, w))
    lib.rtod_plan_destroy(off)
    lib.rtod_plan_destroy(on)


def test_update_conv_errors_without_a_device():
    lib = _ffi.lib()
    h = plan(cfgs.mini_cfg(64, 64), 64)
    (c0, _), (c1, _) = head_layers(h)
    w = np.zeros(255 * 1024, F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rtod_plan_update_conv(None, c0, p(w), p(w)) == -1
    assert lib.rtod_plan_update_conv(h, c0, None, p(w)) == -1 and lib.rtod_plan_update_conv(h, c0, p(w), None) == -1
    assert lib.rtod_plan_update_conv(h, c0 - 1, p(w), p(w)) == -1 and "BatchNorm" in _ffi.last_error()      # a BatchNorm conv
    assert lib.rtod_plan_update_conv(h, c0 + 1, p(w), p(w)) == -1 and "not a convolution" in _ffi.last_error()   # the [yolo] layer
    assert lib.rtod_plan_update_conv(h, -1, p(w), p(w)) == -1 and lib.rtod_plan_update_conv(h, 1000, p(w), p(w)) == -1
    assert lib.rtod_plan_update_conv(h, c0, p(w), p(w)) == -4 and "load_weights" in _ffi.last_error()       # before rtod_plan_load_weights
    assert lib.rtod_plan_update_conv(h, c1, p(w), p(w)) == -4
    lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("precision,options", [(0, ()), (1, ()), (2, ()), (1, (("bn_batch_stats", 1), ("bn_batch_split", 1))), (0, (("bn_batch_stats", 1),))])
def test_pack_of_an_edited_stream_replaces_that_convs_ranges_alone(precision, options):
    """The host-only twin of the device test of rtod_plan_update_conv: both callers of the per-conv pack function go through
    rtod_plan_pack_weights here.  Editing one head conv's block of the stream changes one contiguous run of the image; editing
    every OTHER conv leaves that run as it was; and the image of both edits is the second with the first's run put in."""
    text = cfgs.mini_cfg(64, 64)
    ir = build_ir(parse_cfg_text(text), 64)
    h = plan(text, 64, 4, precision, options)
    w = synth.synth_weights(ir)
    ranges = conv_stream_ranges(ir)
    assert sum(n for _, n, _ in ranges.values()) == w.size
    base = pack(h, w)
    rng = np.random.default_rng(5)
    runs = []
    for conv, _ in head_layers(h):
        off, n, bn = ranges[conv]
        assert not bn
        one = w.copy()
        one[off:off + n] = (w[off:off + n] * F(1.5) + rng.standard_normal(n).astype(F) * F(0.01)).astype(F)
        img = pack(h, one)
        diff = np.flatnonzero(img != base)
        assert len(diff) > n // 4                                     # the edit reaches the image
        lo, hi = int(diff[0]), int(diff[-1]) + 1
        others = w.copy()
        for k, (o, m, _) in ranges.items():
            if k != conv:
                others[o:o + m] = (w[o:o + m] * F(0.75)).astype(F)
        img_o = pack(h, others)
        assert np.array_equal(img_o[lo:hi], base[lo:hi]) and not np.array_equal(img_o, base)
        both = others.copy()
        both[off:off + n] = one[off:off + n]
        want = img_o.copy()
        want[lo:hi] = img[lo:hi]
        assert np.array_equal(pack(h, both), want)
        runs.append((lo, hi))
    assert runs[0][1] <= runs[1][0]                                   # cfg order, disjoint
    _ffi.lib().rtod_plan_destroy(h)


def test_trainer_refuses_v5_heads_and_a_model_without_the_option():
    stub = lambda text, res: types.SimpleNamespace(blocks=parse_cfg_text(text), net_info={"height": res}, input_width=None, options={})
    with pytest.raises(ValueError, match="decode=v5"):
        DarknetTrainer(stub(cfgs.yolov5s_style_cfg(640, 640), 640))
    t = DarknetTrainer(stub(cfgs.mini_cfg(64, 64), 64))
    with pytest.raises(RuntimeError, match="keep_head_inputs"):
        t.head_gradients(np.zeros((1, 3, 64, 64), F), [None])
    with pytest.raises(RuntimeError, match="keep_head_inputs"):
        t.head_step(np.zeros((1, 3, 64, 64), F), [None], 1e-3)
