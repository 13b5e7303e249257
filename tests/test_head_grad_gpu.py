"""GPU tests of the head-gradient path: rtod_yolo_loss_grad (csrc/loss_grad.hip) against the fixture recorded from the reference's
autograd and against tests/head_grad_ref.py, rtod_conv1x1_wgrad (csrc/wgrad.hip) against exact integer and float64 sums,
rtod_plan_update_conv against a full re-pack, option keep_head_inputs, and DarknetTrainer.head_gradients / head_step end to end.

Gates.
* Gradient against the fixture: with D = 2 w (|p| + |t|) s the magnitude the subtraction's operands carry (head_grad_ref.scale), the
  rms and the max of (value - g64) / D over the structurally non-zero elements stay within 4 x the float32 floor recorded with the
  fixture (the reference's own float32 autograd against its float64 autograd; the project's 4 x convention).  The zero pattern is exact.
* Gradient against head_grad_ref on a float32 prediction tensor given to the kernel as it is (so both sides start from the same
  p): g = fl(2w * fl(p - t)) carries two roundings, |error| <= 2u |g| (1 + u) <= 3u D with u = 2^-24 and |p - t| <= |p| + |t|;
  dz = fl(fl(g p) * fl(1 - p)) carries three more, <= 6u D.
* wgrad: integer inputs in [-8, 8] make every product and partial sum an integer below 2^24, so dW and db equal the int64 sums
  bit for bit in any order.  Float inputs: |dW - float64 sum| <= (K - 1) 2^-24 sum |dz| |x| per element, the bound of a K-term fp32
  sum, computed from K.  For K = 1 that bound is 0, which no float32 result of an inexact product can meet: there the test asks
  for the correctly rounded product bit for bit instead (the most any float32 result can give, so it asks no less).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_grad_ref as G
import loss_ref as R
from head_grad_cases import cpu_head_model, fixture_dense, load_grad_cases, wgrad_slices
from loss_cases import bits
from scope_grad_cases import _box, _conv_of, _forward, _model, step_batch
from realtimeobjectdetection_amd import _ffi, cfgs, synth, train as T
from realtimeobjectdetection_amd.util import predict_transform

pytestmark = pytest.mark.gpu
F = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_grad_cases(golden_dir)


def run_grad(pred, images, heads, num_class, min_box=24):
    """One rtod_yolo_loss_grad call through train.yolo_loss_grad_async; everything back on the host, dz also in the row layout."""
    attrs = 5 + num_class
    out = T.yolo_loss_grad_async(pred, [torch.from_numpy(np.asarray(im, F).reshape(-1, attrs)) for im in images], heads, num_class, min_box, grad_pred=True)
    got = {k: v.cpu().numpy() for k, v in out.items() if k != "grad_raw"}
    got["grad_raw"] = [v.cpu().numpy() for v in out["grad_raw"]]
    got["dz_rows"] = np.concatenate([G.rows_from_raw(z, len(an), attrs) for z, (_, _, _, an) in zip(got["grad_raw"], heads)], axis=1)
    loss = T.yolo_loss_async(pred, [torch.from_numpy(np.asarray(im, F).reshape(-1, attrs)) for im in images], heads, num_class, min_box)
    got["loss_components"] = loss["components"].cpu().numpy()
    got["loss_n_obj"] = loss["n_obj"].cpu().numpy()
    return got


# ------------------------------------------------------------------------------------------ 1. the fixture
def test_every_fixture_case_gradient(cases):
    for c in cases:
        dev = [torch.from_numpy(r).cuda() for r in c["raws"]]
        pred = torch.cat([predict_transform(z, 416, an, 80, True, TRAIN=True) for z, (_, _, _, an) in zip(dev, c["heads"])], 1).contiguous()
        got = run_grad(pred, c["images"], c["heads"], 80)
        assert int(got["status"][0]) == 0, c["name"]
        p64 = G.train_decode(c["raws"], c["heads"])
        target, mask, n_obj, _ = R.dense_targets(c["images"], c["heads"], 85)
        assert np.array_equal(got["n_obj"], n_obj) and np.array_equal(np.flatnonzero(mask.reshape(-1)), c["rows"]), c["name"]
        want_g = fixture_dense(c, "g")
        want_g[~mask, 4] = p64[~mask, 4]                              # g_4 = p_4 on a no-object row (pinned in the host tests)
        for which, value, want, floor in (("dz", got["dz_rows"], fixture_dense(c, "dz"), c["grad_floor_dz"]), ("g", got["grad_pred"], want_g, c["grad_floor_g"])):
            assert np.array_equal(value == 0, want == 0), (c["name"], which)             # every element the reference leaves 0 is 0
            assert not np.signbit(value[value == 0]).any(), (c["name"], which)           # ... and stored as +0
            rms, mx = G.relative_error(value, want, G.scale(p64, target, mask, which == "dz"))
            print("%s %s: rms %.3g (floor %.3g)  max %.3g (floor %.3g)" % (c["name"], which, rms, floor[0], mx, floor[1]))
            assert rms <= 4 * floor[0] and mx <= 4 * floor[1], (c["name"], which, rms, mx, floor.tolist())
        assert got["components"].tobytes() == got["loss_components"].tobytes(), c["name"]   # the six doubles of rtod_yolo_loss, bit for bit


# ------------------------------------------------------------------------------------------ 2. odd and rectangular heads
def _geometries():
    rng = np.random.default_rng(17)
    rnd = lambda H, W, C_, n: [_box(rng.uniform(0, W - 0.01), rng.uniform(0, H - 0.01), rng.uniform(6, W), rng.uniform(6, H), C_, 0 if C_ == 1 or rng.random() < 0.8 else 1) for _ in range(n)]
    none = lambda C_: np.zeros((0, 5 + C_), F)
    return {
        # name: (heads, classes, images, min_box, status)
        "g2x2_a1_c1": ([(2, 2, 32, [(40, 50)])], 1, [np.stack([_box(40, 41, 30, 30, 1), _box(45, 47, 50, 20, 1)]), none(1)], 4, 0),      # two boxes on one (cell, anchor); no boxes
        "g3x5_a3_c80": ([(3, 5, 32, [(10, 14), (23, 27), (37, 58)])], 80, [np.stack(rnd(96, 160, 80, 9) + [_box(170, 20, 30, 30, 80), _box(20, -1, 30, 30, 80)]), np.stack(rnd(96, 160, 80, 4))], 4, 1),
        "g13_a3_g2_a1_c1": ([(13, 13, 8, [(10, 13), (16, 30), (33, 23)]), (2, 2, 52, [(60, 60)])], 1, [np.stack(rnd(104, 104, 1, 30)), none(1), np.stack(rnd(104, 104, 1, 3))], 4, 0),
        "g13_a3_c80_b2": ([(13, 13, 32, [(116, 90), (156, 198), (373, 326)])], 80, [np.stack(rnd(416, 416, 80, 12)), np.stack(rnd(416, 416, 80, 5))], 24, 0),
    }


@pytest.mark.parametrize("name", ["g2x2_a1_c1", "g3x5_a3_c80", "g13_a3_g2_a1_c1", "g13_a3_c80_b2"])
def test_odd_and_rectangular_heads_against_head_grad_ref(name):
    heads, C_, images, min_box, status = _geometries()[name]
    attrs, B = 5 + C_, len(images)
    rng = np.random.RandomState(len(name))
    raws = [rng.standard_normal((B, len(an) * attrs, gh, gw)).astype(F) for gh, gw, _, an in heads]
    pred = G.train_decode(raws, heads).astype(F)                      # a float32 tensor both sides start from
    got = run_grad(torch.from_numpy(pred).cuda(), images, heads, C_, min_box)
    target, mask, n_obj, st = R.dense_targets(images, heads, attrs, min_box)
    assert st == status and int(got["status"][0]) == status and np.array_equal(got["n_obj"], n_obj) and mask.any(), name
    if name == "g2x2_a1_c1":
        assert int(n_obj[0]) == 1 and np.array_equal(target[0][mask[0]][0, 4:], images[0][1][4:])      # the later box owns the row
    p64 = pred.astype(np.float64)
    for which, value, want, k in (("g", got["grad_pred"], G.grad_pred(p64, target, mask), 3), ("dz", got["dz_rows"], G.grad_raw_rows(p64, target, mask), 6)):
        d = G.scale(p64, target, mask, which == "dz")
        assert np.array_equal(value == 0, want == 0) and not np.signbit(value[value == 0]).any(), (name, which)
        assert (np.abs(value - want) <= k * U * d).all(), (name, which, float((np.abs(value - want) / np.where(d == 0, 1, d)).max() / U))
    assert got["components"].tobytes() == got["loss_components"].tobytes() and np.array_equal(got["n_obj"], got["loss_n_obj"]), name
    flat = np.concatenate([z.reshape(-1) for z in got["grad_raw"]])   # the documented head offsets: head h behind batch * the earlier heads
    assert got["grad_raw_flat"].tobytes() == flat.tobytes() and flat.size == B * mask.shape[1] * attrs, name


# ------------------------------------------------------------------------------------------ 3 / 4. the weight gradient
WGRAD_SHAPES = [(1, 1, 32, 1), (1, 255, 32, 4), (3, 255, 96, 169), (2, 24, 64, 676), (8, 255, 1024, 4)]


def _wgrad(dz, x):
    B, cout, P = dz.shape
    dw, db = T.conv1x1_wgrad_async(torch.from_numpy(dz).cuda().view(B, cout, P, 1), torch.from_numpy(x).cuda().view(B, x.shape[1], P, 1))
    return dw.cpu().numpy().reshape(cout, x.shape[1]), db.cpu().numpy()


def test_wgrad_shapes_span_the_slice_rule():
    S = [wgrad_slices(B * P)[0] for B, _, _, P in WGRAD_SHAPES]
    assert S[0] == 1 and S[1] == 1 and S[2] > 1 and S[3] > 1 and S[4] > 1, S   # the last two (and the third) span several K slices
    assert wgrad_slices(2 * 676)[1] % 32 != 0                                  # ... with a slice length that is no multiple of the staged chunk


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_exact_on_small_integers(shape):
    B, cout, cin, P = shape
    rng = np.random.default_rng(B * 1000 + P)
    dz, x = rng.integers(-8, 9, (B, cout, P)), rng.integers(-8, 9, (B, cin, P))
    assert 64 * B * P < 2 ** 24
    dw, db = _wgrad(dz.astype(F), x.astype(F))
    assert np.array_equal(dw.astype(np.int64), np.einsum("bop,bcp->oc", dz, x)) and np.array_equal(dw, np.rint(dw)), shape
    assert np.array_equal(db.astype(np.int64), dz.sum(axis=(0, 2))), shape


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_floats_within_the_summation_bound_and_reproducible(shape):
    B, cout, cin, P = shape
    K = B * P
    rng = np.random.default_rng(B * 77 + P)
    dz, x = rng.standard_normal((B, cout, P)).astype(F), rng.standard_normal((B, cin, P)).astype(F)
    dw, db = _wgrad(dz, x)
    want = np.einsum("bop,bcp->oc", dz.astype(np.float64), x.astype(np.float64))
    if K == 1:                                                        # the bound is 0: the correctly rounded product, bit for bit
        assert np.array_equal(bits(dw), bits(want.astype(F))), shape
    else:
        bound = (K - 1) * U * np.einsum("bop,bcp->oc", np.abs(dz).astype(np.float64), np.abs(x).astype(np.float64))
        assert (np.abs(dw - want) <= bound).all(), (shape, float((np.abs(dw - want) / bound).max()))
    assert (np.abs(db - dz.astype(np.float64).sum(axis=(0, 2))) <= (K - 1) * U * np.abs(dz).astype(np.float64).sum(axis=(0, 2))).all(), shape
    dw2, db2 = _wgrad(dz, x)
    assert dw.tobytes() == dw2.tobytes() and db.tobytes() == db2.tobytes(), shape


# ------------------------------------------------------------------------------------------ 5. update_conv
@pytest.mark.parametrize("precision,train", [("fp32", False), ("f16s3", False), ("f16", False), ("f16s3", True)])
def test_update_conv_packs_like_load_weights(tmp_path, precision, train):
    res, B = 64, 2
    text = cfgs.mini_cfg(res, res)
    options = {"bn_batch_split": 1} if train else {}
    m = _model(tmp_path, text, res, precision, options, train, keep_all=True)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=3)).cuda()
    lib = _ffi.lib()
    heads = m.head_layers()
    assert heads == [(14, 13), (22, 21)]
    w0 = _conv_of(m, 14).weight.detach().clone()
    assert lib.rtod_plan_update_conv(None, 14, None, None) == -1
    before = _forward(m, x)
    assert m.active_precision == precision
    n_layers = len(m.module_list)
    readable = [i for i in range(n_layers) if lib.rtod_plan_layer_shape(m._plan, i, C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_int())) == 0]
    layers_before = {i: m.read_layer(i, B) for i in readable}
    wz = np.zeros(w0.numel(), F)
    assert lib.rtod_plan_update_conv(m._plan, 13, wz.ctypes.data_as(C.c_void_p), wz.ctypes.data_as(C.c_void_p)) == -1 and "BatchNorm" in _ffi.last_error()
    rng = np.random.default_rng(8)
    version = (m._weights_version, m._plan_weights_version)
    for layer, _ in heads:
        conv = _conv_of(m, layer)
        m.update_conv(layer, conv.weight.detach() * 1.25 + torch.from_numpy(rng.standard_normal(tuple(conv.weight.shape)).astype(F)) * 0.01,
                      conv.bias.detach() - 0.5)
    assert (m._weights_version, m._plan_weights_version) == version and not torch.equal(_conv_of(m, 14).weight, w0)   # no full re-pack is due
    plan_handle = m._plan.value
    after = _forward(m, x)
    assert m._plan.value == plan_handle and not torch.equal(after, before)
    fresh = _model(tmp_path, text, res, precision, options, train, keep_all=True, weights=m.weight_stream(), name="fresh")
    want = _forward(fresh, x)
    assert np.array_equal(bits(after.cpu().numpy()), bits(want.cpu().numpy()))
    # every other conv computes what it computed before, and what the freshly packed plan computes
    for i in readable:
        now = m.read_layer(i, B)
        assert torch.equal(now, fresh.read_layer(i, B)), i
        assert torch.equal(now, layers_before[i]) or i in (14, 15, 22, 23), i


def test_update_conv_before_loading_is_a_state_error(tmp_path):
    from head_grad_cases import plan
    h = plan(cfgs.mini_cfg(64, 64), 64)
    w = np.zeros(255 * 1024, F)
    assert _ffi.lib().rtod_plan_update_conv(h, 14, w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)) == -4
    _ffi.lib().rtod_plan_destroy(h)


# ------------------------------------------------------------------------------------------ 6. keep_head_inputs
@pytest.mark.parametrize("net,precision", [("mini", "fp32"), ("mini", "f16s3"), ("mini", "f16"), ("fallback", "fp32")])
def test_keep_head_inputs_changes_nothing_but_liveness(tmp_path, net, precision):
    res, B = 64, 3
    text = cfgs.mini_cfg(res, res) if net == "mini" else cfgs.mini_fallback_cfg(res, res)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=6)).cuda()
    off = _model(tmp_path, text, res, precision, name="off")
    on = _model(tmp_path, text, res, precision, {"keep_head_inputs": 1}, name="on")
    every = _model(tmp_path, text, res, precision, keep_all=True, name="all")
    for td in (False, True):
        y_off, y_on, y_all = _forward(off, x, td), _forward(on, x, td), _forward(every, x, td)
        assert np.array_equal(bits(y_off.cpu().numpy()), bits(y_on.cpu().numpy())) and np.array_equal(bits(y_off.cpu().numpy()), bits(y_all.cpu().numpy()))
        for _, inp in on.head_layers():
            got, want = on.read_layer(inp, B), every.read_layer(inp, B)
            assert got.abs().sum() > 0 and torch.equal(got, want), (net, precision, inp)
    assert [li.variant for li in off.launch_infos()] == [li.variant for li in on.launch_infos()]
    assert on._info.arena_bytes >= off._info.arena_bytes


# ------------------------------------------------------------------------------------------ 7 / 8. end to end
def _trainer(tmp_path, precision):
    m = _model(tmp_path, cfgs.mini_cfg(64, 64), 64, precision, {"keep_head_inputs": 1})
    t = T.DarknetTrainer(m)
    t.min_box_size = 4
    return m, t


def _head_state(m, B):
    xs = [m.read_layer(inp, B).cpu().numpy().astype(np.float64) for _, inp in m.head_layers()]
    ws = [_conv_of(m, c).weight.detach().cpu().numpy().astype(np.float64) for c, _ in m.head_layers()]
    bs = [_conv_of(m, c).bias.detach().cpu().numpy().astype(np.float64) for c, _ in m.head_layers()]
    return xs, ws, bs


@pytest.mark.parametrize("precision", ["fp32", "f16s3"])
def test_head_gradients_against_autograd(tmp_path, cases, precision):
    """dW, db of DarknetTrainer.head_gradients against torch autograd of a float64 CPU model of the heads (conv2d on the device's own
    head inputs X from read_layer and the model's head weights, the TRAIN decode restated, the loss on tests/loss_ref.py's targets).

    Bound per element of dW, with K = B * GH * GW (12 and 48 here), x the head input and u = 2^-24.  The device sums fl(dz_dev * x) in
    fp32: by the gate of the float wgrad test its result is within (K - 1) u sum |dz_dev| |x| of the exact sum of its own operands.
    Its operand dz_dev differs from the float64 dz by at most 4 F D per element, F the recorded float32 floor (max form, the largest
    over the fixture's cases) and D = 2 w (|p| + |t|) s from the CPU model: the gate of the fixture test.  So
      |dW_dev - dW_64| <= (K - 1) u sum |dz_64| |x|  +  (1 + (K - 1) u) sum 4 F D |x|,
    and for db the same with |x| = 1.  The second factor covers the first term's use of dz_dev instead of dz_64."""
    B = 3
    m, t = _trainer(tmp_path, precision)
    # the synthetic head weights give raw values up to |z| = 47, where a float32 sigmoid is exactly 1 and the float32 gradient exactly 0;
    # the floor F was recorded on standard-normal maps (|z| < 5.5).  A tenth of the head weights keeps the test where F was measured
    for layer, _ in m.head_layers():
        m.update_conv(layer, _conv_of(m, layer).weight.detach() * 0.1, _conv_of(m, layer).bias.detach() * 0.1)
    x, images = step_batch()
    loss, grads = t.head_gradients(torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images])
    assert m.active_precision == precision and int(t.status.item()) == 0 and sorted(grads) == [14, 22]
    xs, ws, bs = _head_state(m, B)
    assert [a.shape for a in xs] == [(3, 1024, 2, 2), (3, 512, 4, 4)]
    cpu = cpu_head_model(xs, ws, bs, t.heads, images, 4)
    assert cpu["status"] == 0 and cpu["mask"].any()
    floor = max(float(c["grad_floor_dz"][1]) for c in cases)
    d_rows = G.scale(cpu["pred"], cpu["target"], cpu["mask"], True)
    comp = t.last_components.cpu().numpy()
    assert float(loss) == float(F(comp[0])) and abs(comp[0] - cpu["loss"]) <= 1e-4 * cpu["loss"]
    for h, ((layer, _), d_map) in enumerate(zip(m.head_layers(), G.split_heads(d_rows, t.heads))):
        dw, db = (v.cpu().numpy().astype(np.float64) for v in grads[layer])
        assert dw.shape == ws[h].shape and db.shape == bs[h].shape
        K = B * xs[h].shape[2] * xs[h].shape[3]
        ax, adz = np.abs(xs[h]), np.abs(cpu["dz"][h])
        bound_w = (K - 1) * U * np.einsum("bohw,bchw->oc", adz, ax) + (1 + (K - 1) * U) * 4 * floor * np.einsum("bohw,bchw->oc", d_map, ax)
        bound_b = (K - 1) * U * adz.sum(axis=(0, 2, 3)) + (1 + (K - 1) * U) * 4 * floor * d_map.sum(axis=(0, 2, 3))
        ew, eb = np.abs(dw[:, :, 0, 0] - cpu["dw"][h][:, :, 0, 0]), np.abs(db - cpu["db"][h])
        ratio = lambda e, b: float(np.divide(e, b, out=np.zeros_like(e), where=b > 0).max())   # a bound of 0: a channel whose gradient is structurally 0
        print("%s head %d (K = %d): dW worst error / bound %.3g, db %.3g" % (precision, h, K, ratio(ew, bound_w), ratio(eb, bound_b)))
        assert (ew <= bound_w).all() and (eb <= bound_b).all(), (precision, h)
        assert np.abs(cpu["dw"][h]).max() > 0


EPS = 1e-4


def test_the_step_descends_by_what_the_gradient_says(tmp_path):
    """The central difference of the device loss along -g, (L(w + eps g) - L(w - eps g)) / (2 eps) with the weights moved by
    update_conv, against ||g||^2 of head_gradients (fp32 plan, mini_cfg(64, 64), the batch of step_batch).

    eps and the allowed gap come from a float64 CPU model of the same heads (head_grad_cases.cpu_head_model on the CPU oracle's head
    inputs for this batch and these weights), run without a device while writing the test.  There the loss is 709.77 and
    ||g||^2 = 5.1808e6; the central difference misses ||g||^2 by 6.16e8 eps^2 (573 at eps = 1e-3, 6.16 at 1e-4, 0.0616 at 1e-5: the
    cubic term of the loss along g), and the loss of the same heads evaluated in float32 differs from the float64 loss by 4.4e-5, which
    a difference quotient divides by eps (0.44 at 1e-4, 4.4 at 1e-5).  eps = 1e-4 is the smallest of these steps at which the
    modelled truncation term still exceeds the noise term tenfold, so the gap is a figure the model predicts (1.2e-6 of ||g||^2)
    rather than noise; at 3e-4 a plain SGD step already overshoots (the loss rises), at 1e-4 three steps of the CPU model fall
    709.77 -> 391.57 -> 343.79 -> 318.70.  The test recomputes both numbers from the CPU model on the device's own head inputs and
    allows    4 * |fd_cpu - ||g_cpu||^2|  +  2 * noise / (2 eps),     noise = |L_cpu,float32 - L_cpu,float64|,
    one noise per loss evaluation.  Neither number was adjusted to a device result.  Then three head_step calls at lr = eps on the
    same batch: the loss falls each time."""
    B = 3
    m, t = _trainer(tmp_path, "fp32")
    x, images = step_batch()
    xd, bnd = torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images]
    loss0, grads = t.head_gradients(xd, bnd)
    l0 = float(t.last_components[0].item())
    g2 = sum(float((dw.double() ** 2).sum() + (db.double() ** 2).sum()) for dw, db in grads.values())
    xs, ws, bs = _head_state(m, B)
    cpu = cpu_head_model(xs, ws, bs, t.heads, images, 4)
    g2_cpu = sum(float((a ** 2).sum()) for a in cpu["dw"] + cpu["db"])
    shifted = lambda s: cpu_head_model(xs, [w + s * g for w, g in zip(ws, cpu["dw"])], [b + s * g for b, g in zip(bs, cpu["db"])], t.heads, images, 4)["loss"]
    gap_cpu = abs((shifted(EPS) - shifted(-EPS)) / (2 * EPS) - g2_cpu)
    f32 = lambda arrs: [a.astype(F) for a in arrs]
    noise = abs(cpu_head_model(f32(xs), f32(ws), f32(bs), t.heads, images, 4, torch.float32)["loss"] - cpu["loss"])
    allowed = 4 * gap_cpu + 2 * noise / (2 * EPS)
    masters = {layer: (_conv_of(m, layer).weight.detach().clone().cuda(), _conv_of(m, layer).bias.detach().clone().cuda()) for layer in grads}

    def loss_at(s):
        for layer, (dw, db) in grads.items():
            m.update_conv(layer, masters[layer][0] + s * dw, masters[layer][1] + s * db)
        t.forward_loss(xd, bnd)
        return float(t.last_components[0].item())
    fd = (loss_at(EPS) - loss_at(-EPS)) / (2 * EPS)
    assert loss_at(0.0) == l0                                         # the weights are back, bit for bit
    print("||g||^2 device %.8g cpu %.8g; central difference device %.8g; |fd - ||g||^2| %.4g, allowed %.4g (cpu gap %.4g, noise %.4g)"
          % (g2, g2_cpu, fd, abs(fd - g2), allowed, gap_cpu, noise))
    assert g2 > 0 and abs(fd - g2) <= allowed
    losses = [float(t.head_step(xd, bnd, EPS)) for _ in range(3)]
    t.forward_loss(xd, bnd)
    losses.append(float(t.last_components[0].item()))
    assert losses[0] == float(F(l0)) and losses[0] > losses[1] > losses[2] > losses[3], losses
