"""GPU tests of training under batch statistics on the split-f16 kernels: a model in .train() with precision "f16s3" and options
bn_batch_split + keep_bn_inputs + the keep option of the scope.  mini_cfg at 64 x 64, batch 3, scope "backbone", and the square probes
of tests/bn_split_model.py.  Run on an MI355X with ``pytest -m gpu``.

1. The forward with keep_bn_inputs is the forward without it, bit for bit, on every legal tile of every probe; read_bn_input is what
   the plan's statistics were taken of and what its normalise step stored.
2. batchnorm_gradients against float64 autograd of the sub-graph with training=True BatchNorm whose VALUES are pinned to the device's:
   pin(value, device) = device + (value - value.detach()) has the device's value (the split forward's, format error and all) and the
   model's derivative.  With the values pinned the device backward is the exact-fp32 path's arithmetic, so the gate is that path's: rms
   and max of the error within 4 x float32 torch's on the same pinned graph.
4. - 6. The training step: masters, moments, the packed image, the next forward, determinism, the optimiser round trip.
7. The loss falls along the gradient by what the gradient says (tests/test_bn_train_gpu.py's recipe and bound).
(3., the distance of these gradients from the exact-fp32 batch plan's, is recorded by tools/exp_bn_grad_split.py, not gated.)"""
import numpy as np
import pytest
import torch

from block_grad_cases import opt_update_f32
from bn_grad_cases import fma32, plan_stats
from bn_split_model import SQUARE
from conv_probes import FAMILIES, accepted_ids, launch_of_layer, setup
from f16s3_emulation import store_split_f32
from full_grad_cases import full_batch
from head_grad_cases import cpu_head_model, pack
from loss_cases import bits
from scope_grad_cases import KEEP, _bn_of, _conv_of, _forward, _frames, _model, _same, _t64, tenth_heads
from realtimeobjectdetection_amd import _ffi, cfgs, train as T
from realtimeobjectdetection_amd.cfg import build_ir
from test_bn_train_gpu import cpu_graph_bn

pytestmark = pytest.mark.gpu
F = np.float32
fn = torch.nn.functional
B = 3
SCOPE = "backbone"
OPTIONS = dict(KEEP[SCOPE], bn_batch_split=1, keep_bn_inputs=1)
PLAIN = dict(KEEP[SCOPE], bn_batch_split=1)
PROBES = [p for p in SQUARE]


def _mini(tmp_path, name="m", options=OPTIONS, precision="f16s3", running=False, keep_all=False, text=None, res=64):
    m = _model(tmp_path, cfgs.mini_cfg(64, 64) if text is None else text, res, precision, options, train=True, keep_all=keep_all, name=name)
    m.update_running_stats = running
    return m


def _trainer(tmp_path, name="m", options=OPTIONS, precision="f16s3", running=False):
    m = _mini(tmp_path, name, options, precision, running)
    t = T.DarknetTrainer(m, trainable=SCOPE)
    t.min_box_size = 4
    images = full_batch(64, 64, 80, B)
    return m, t, _frames(B, 64, None), [torch.from_numpy(im) for im in images], images


def _host(a):
    return None if a is None else a.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the forward
def _split_normalise(z, mean, var, gamma, beta, leaky):
    """The normalise step of the split plans on the raw sums ``z`` [B,C,H,W] (aux_kernels.hip bn_channel_constants, bn_normalise and the
    split store): w and b in double, rounded to float once each, u = fma(z, w, b), leaky: u > 0 ? u : u * 0.1f, then 8 u as f16 hi + lo;
    the value read_layer returns is (hi + lo) / 8."""
    r = 1.0 / np.sqrt(np.asarray(var, np.float64) + 1e-5)
    w = (r * gamma.astype(np.float64)).astype(F)
    b = (beta.astype(np.float64) - np.asarray(mean, np.float64) * r * gamma.astype(np.float64)).astype(F)
    u = fma32(z, w.reshape(1, -1, 1, 1), b.reshape(1, -1, 1, 1))
    u = np.where(u > 0, u, u * F(0.1)).astype(F) if leaky else u
    return store_split_f32(torch.from_numpy(np.ascontiguousarray(u))).numpy().astype(F)


def _check_kept_inputs(tag, kept, listed, leaky_of, params_of, batch):
    """read_bn_input of every listed conv: the plan's statistics are its float64 mean and biased variance (the double-sum bound of
    tests/test_bn_grad_gpu.py), and the split normalise of it is the stored map, bit for bit."""
    for c in listed:
        z = kept.read_bn_input(c, batch).cpu().numpy()
        mean, var = plan_stats(kept, c, z.shape[1])
        gamma, beta = params_of(c)
        z64 = z.astype(np.float64)
        assert np.isfinite(z).all() and np.abs(z).max() > 0, (tag, c)
        assert np.allclose(mean, z64.mean(axis=(0, 2, 3)), rtol=0, atol=1e-12 * np.abs(z).max()), (tag, c)
        assert (np.abs(var - z64.var(axis=(0, 2, 3))) <= 1e-9 * (var + mean * mean)).all(), (tag, c)
        want = _split_normalise(z, mean, var, gamma, beta, leaky_of(c))
        got = kept.read_layer(c, batch).cpu().numpy()
        wrong = int((bits(got) != bits(want)).sum())
        if wrong:
            print("%s conv %d: %d of %d stored values differ from the split normalise of read_bn_input" % (tag, c, wrong, got.size))
        assert wrong == 0, (tag, c, wrong)


def _stored(m, batch):
    torch.cuda.synchronize()
    out = {}
    for D in m.plan_description()["layers"]:
        if D["type"] == "yolo" or (D["type"] == "convolutional" and D["fused_into"] >= 0):
            continue
        out[D["index"]] = m.read_layer(D["index"], batch).cpu()
    return out


def test_mini_forward_with_kept_inputs_is_the_forward_without_them(tmp_path):
    x = _frames(B, 64, None)
    kept, plain = _mini(tmp_path, "kept", keep_all=True), _mini(tmp_path, "plain", PLAIN, keep_all=True)
    y1, y0 = _forward(kept, x), _forward(plain, x)
    assert kept.active_precision == plain.active_precision == "f16s3" and kept.plan_description()["bn_batch_trained"] == "split"
    assert _same(y1, y0) and not kept.overflowed()
    s1, s0 = _stored(kept, B), _stored(plain, B)
    assert s1.keys() == s0.keys() and all(torch.equal(s1[i], s0[i]) for i in s1)
    listed = [c for c, _ in kept.trainable_layers()]
    assert len(listed) == 14 and plain.trainable_layers() == []
    with pytest.raises(Exception, match="keep_bn_inputs"):
        plain.read_bn_input(listed[0], B)
    ir = {L.index: L for L in build_ir(kept.blocks, 64).layers}
    tiles = {li.layer: li.variant - 100 for li in kept.launch_infos() if li.kind == 0 and li.variant >= 100}
    fams = sorted({f for c in listed for f, r in FAMILIES.items() if tiles[c] in r})
    print("mini_cfg: tile of every trained conv %s, families %s" % ({c: tiles[c] for c in listed}, fams))
    _check_kept_inputs("mini", kept, listed, lambda c: ir[c].leaky,
                       lambda c: (_host(_bn_of(kept, c).weight), _host(_bn_of(kept, c).bias)), B)
    # the same forward without keep_all_layers (the plan a trainer runs): the same output, the same kept rows
    lean = _mini(tmp_path, "lean")
    assert _same(_forward(lean, x), y1)
    for c in listed[:1] + listed[-1:]:
        assert _same(lean.read_bn_input(c, B), kept.read_bn_input(c, B)) and _same(lean.read_layer(c, B), kept.read_layer(c, B)), c


@pytest.mark.parametrize("name", [p.name for p in PROBES])
def test_probe_every_legal_tile_keeps_the_bits_and_the_inputs(tmp_path, name):
    from test_bn_split_gpu import _model as probe_model
    p = next(q for q in PROBES if q.name == name)
    ref, wts, x = setup(p)
    xg = x.cuda()
    (tmp_path / "kept").mkdir()
    (tmp_path / "plain").mkdir()
    kept = probe_model(p.cfg(), p.H, tmp_path / "kept", wts, dict(p.options, **OPTIONS))
    plain = probe_model(p.cfg(), p.H, tmp_path / "plain", wts, dict(p.options, **PLAIN))
    for m in (kept, plain):
        m.prepare(p.B, xg.device)
        assert m.active_precision == "f16s3"
    n = kept._info.n_launches
    launch = launch_of_layer(kept.launch_infos(), p.conv_layer)
    assert n == plain._info.n_launches and launch == launch_of_layer(plain.launch_infos(), p.conv_layer)
    ids = accepted_ids(_ffi.lib(), kept._plan, n, launch, p.B)
    assert ids and ids == accepted_ids(_ffi.lib(), plain._plan, n, launch, p.B)
    listed = [c for c, _ in kept.trainable_layers()]
    assert (listed == [] and p.act == "silu") or p.conv_layer in listed, (name, listed)     # SiLU has no backward: nothing of that probe is trained
    fams = sorted(f for f, r in FAMILIES.items() if set(ids) & set(r))
    print("PROBE %s (%s): trained %s, families %s, ids %s" % (name, p.note, listed, fams, ids))
    layers = ref.ir.layers
    for v in ids:
        table = [-1] * n
        table[launch] = v
        for m in (kept, plain):
            m.set_tiles(p.B, table)
        with torch.no_grad():
            y1, y0 = kept(xg).clone(), plain(xg).clone()
        assert kept.launch_infos()[launch].variant == 100 + v == plain.launch_infos()[launch].variant, (name, v)
        s1, s0 = _stored(kept, p.B), _stored(plain, p.B)
        assert torch.equal(y1, y0) and s1.keys() == s0.keys() and all(torch.equal(s1[i], s0[i]) for i in s1), (name, v)
        _check_kept_inputs("%s tile %d" % (name, v), kept, listed, lambda c: layers[c].leaky,
                           lambda c: (ref.params[c]["gamma"].numpy().astype(F), ref.params[c]["beta"].numpy().astype(F)), p.B)
    assert not kept.overflowed()


# ---------------------------------------------------------------------------------------------- 2. the gradients
def _pin(value, device_value):
    """The device's value with the model's derivative."""
    return device_value.to(value.dtype) + (value - value.detach())


def pinned_grads(m, t, dtype, masks, dzs, z_dev, stored):
    """autograd of the scope's sub-graph in ``dtype`` with training=True BatchNorm, every BatchNorm conv's z and every member's stored
    value pinned to the device's, the device's leaky masks: {conv: (dW, dgamma, dbeta)} as float64 numpy."""
    layers, readers, member, scales = t._graph(SCOPE)
    cast = lambda a: torch.as_tensor(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).to(dtype)
    val, leaves = {}, {}

    def value(src):
        if src not in val:
            assert not member[src]
            val[src] = cast(stored[src])
        return val[src]

    for L in layers:
        i = L.index
        if not member[i]:
            continue
        if L.type == "convolutional":
            conv, x = _conv_of(m, i), value(i - 1)
            if i in scales:
                bn = _bn_of(m, i)
                W, g, b = (cast(p).requires_grad_(True) for p in (conv.weight, bn.weight, bn.bias))
                leaves[i] = (W, g, b)
                z = _pin(fn.conv2d(x, W, stride=L.stride, padding=L.size // 2), cast(z_dev[i]))
                u = fn.batch_norm(z, None, None, g, b, True, 0.0, 1e-5)
                val[i] = _pin(u * cast(masks[i]) if L.leaky else u, cast(stored[i]))
            else:
                val[i] = fn.conv2d(x, cast(conv.weight), cast(conv.bias))       # a head conv: its raw map is not stored
            continue
        if L.type == "upsample":
            v = fn.interpolate(value(i - 1), scale_factor=2, mode="nearest") if L.nearest else fn.interpolate(value(i - 1), scale_factor=2, mode="bilinear", align_corners=False)
        elif L.type == "shortcut":
            v = value(L.srcs[0]) + value(L.srcs[1])
        else:
            parts, off = [], 0
            for s in L.srcs:
                parts.append(value(s) if member[s] else cast(stored[i])[:, off:off + layers[s].cout])
                off += layers[s].cout
            v = torch.cat(parts, 1)
        val[i] = _pin(v, cast(stored[i]))
    sum((val[head] * dz.detach().cpu().to(dtype)).sum() for (head, _), dz in zip(m.head_layers(), dzs)).backward()
    return {i: tuple(p.grad.numpy().astype(np.float64) for p in ps) for i, ps in leaves.items()}


def test_batchnorm_gradients_against_pinned_autograd(tmp_path):
    """dW, dgamma and dbeta of every listed conv of mini_cfg against the pinned float64 graph; the floor is float32 torch on the same
    pinned graph.  Prints the measured multiple of the floor per conv and parameter before it asserts that none exceeds 4.  A second call
    repeats every bit (5., gradients).

    Measured on an MI355X, worst multiple over the 14 convs and the three parameters: rms 1.77, max 2.25 (both at conv 12)."""
    m, t, xd, bnd, _ = _trainer(tmp_path)
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads, bn_grads = t.batchnorm_gradients(xd, bnd)
    listed = [c for c, _ in m.trainable_layers()]
    assert m.active_precision == "f16s3" and int(t.status.item()) == 0 and len(listed) == 14 and sorted(grads) == sorted(bn_grads) == listed
    assert not m.overflowed()
    loss2, heads2, again, bn_again = t.batchnorm_gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(grads[k], again[k]) and _same(bn_grads[k][0], bn_again[k][0]) and _same(bn_grads[k][1], bn_again[k][1]) for k in grads)
    assert all(_same(head_grads[k][0], heads2[k][0]) and _same(head_grads[k][1], heads2[k][1]) for k in heads2)
    layers, readers, member, scales = t._graph(SCOPE)
    assert all(s is None for s in scales.values())
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    need = {i for i in range(len(layers)) if member[i] and not (layers[i].type == "convolutional" and i not in scales)}
    need |= {s for i in range(len(layers)) if member[i] for s in ((layers[i].srcs if layers[i].type in ("route", "shortcut") else (i - 1,))) if s >= 0}
    stored = {i: m.read_layer(i, B).cpu() for i in sorted(need)}
    z_dev = {c: m.read_bn_input(c, B).cpu() for c in listed}
    masks = {c: np.where(stored[c].numpy() > 0, 1.0, 0.1) for c in listed if layers[c].leaky}
    want = pinned_grads(m, t, torch.float64, masks, dzs, z_dev, stored)
    floor = pinned_grads(m, t, torch.float32, masks, dzs, z_dev, stored)
    over, worst = [], [0.0, 0.0]
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    for c in listed:
        got = (grads[c], bn_grads[c][0], bn_grads[c][1])
        for name, g, w, f in zip(("dW", "dgamma", "dbeta"), got, want[c], floor[c]):
            g, ref = g.cpu().numpy().astype(np.float64), np.abs(w).max()
            assert g.shape == w.shape and ref > 0, (c, name)
            e_dev, e_32 = (g - w) / ref, (f - w) / ref
            q_rms, q_max = rms(e_dev) / rms(e_32), float(np.abs(e_dev).max() / np.abs(e_32).max())
            worst = [max(worst[0], q_rms), max(worst[1], q_max)]
            print("split conv %d %s: rms %.3g (floor %.3g, ratio %.2f)  max %.3g (floor %.3g, ratio %.2f)" % (
                c, name, rms(e_dev), rms(e_32), q_rms, np.abs(e_dev).max(), np.abs(e_32).max(), q_max))
            if not (q_rms <= 4 and q_max <= 4):
                over.append((c, name, round(q_rms, 2), round(q_max, 2)))
    print("split mini-backbone: worst rms ratio %.2f, worst max ratio %.2f" % tuple(worst))
    assert not over, ("(conv, parameter, rms ratio, max ratio) over 4 x the float32 floor", over)


# ---------------------------------------------------------------------------------------------- 4. the training step
NAMES = (("weight", ""), ("bias", "_bias"), ("bn_weight", "_bn_weight"), ("bn_bias", "_bn_bias"))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_training_steps_on_the_split_plan(tmp_path, kind):
    """Three feed_forward_through_model steps (lr 1e-4).  After each: masters and moments of conv weight, gamma and beta (and of the heads'
    weight and bias) equal opt_update_f32 of the gradients batchnorm_gradients returned for the state before the step, bit for bit; the
    packed image equals the host pack of the synchronised parameters, bit for bit; running_mean / running_var are what the forward alone
    leaves (a twin that only runs forwards).  After the first and the third step the next forward equals that of a fresh model built
    from state_dict(), bit for bit."""
    m, t, xd, bnd, _ = _trainer(tmp_path, running=True)
    twin = _trainer(tmp_path, "twin", running=True)[0]
    t.optimizer = T.HeadOptimizer(kind, lr=1e-4)
    losses = []
    for step in range(3):
        m.update_running_stats = False                                # (the gradients below are a look, not a step)
        _, hg, ng, bg = t.batchnorm_gradients(xd, bnd)
        m.update_running_stats = True
        grads = {k: (_host(dw), _host(db), None, None) for k, (dw, db) in hg.items()}
        grads.update({k: (_host(dw), None, _host(bg[k][0]), _host(bg[k][1])) for k, dw in ng.items()})
        masters = t._masters(list(hg) + list(ng), xd.device)
        before = {k: tuple(_host(p) for p in (list(masters[k]) + [None, None])[:4]) for k in grads}
        state = {k: {n: _host(v) for n, v in t.optimizer.state.get(k, {}).items() if n.startswith("exp_avg")} for k in grads}
        if step:
            for c in ng:
                twin.update_conv_bn(c, *[torch.from_numpy(p) for p in (before[c][0], before[c][2], before[c][3])])
            for h_ in hg:
                twin.update_conv(h_, torch.from_numpy(before[h_][0]), torch.from_numpy(before[h_][1]))
        losses.append(float(t.feed_forward_through_model(xd, bnd)))
        with twin.train_mode():
            _forward(twin, xd)
        for k in grads:
            st = t.optimizer.state[k]
            assert st["step"] == step + 1 and st["weight"] is t._head_masters[k][0]
            for which, (name, sfx) in enumerate(NAMES):
                if before[k][which] is None:
                    assert name not in st
                    continue
                zero = np.zeros_like(before[k][which])
                w1, m1, v1 = opt_update_f32(kind, before[k][which], grads[k][which], state[k].get("exp_avg" + sfx, zero), state[k].get("exp_avg_sq" + sfx, zero),
                                            1e-4, step=st["step"])
                assert np.array_equal(bits(_host(st[name])), bits(w1)), (step, k, name)
                if kind == "adam":
                    assert np.array_equal(bits(_host(st["exp_avg" + sfx])), bits(m1)) and np.array_equal(bits(_host(st["exp_avg_sq" + sfx])), bits(v1)), (step, k, name)
        image = m.packed_weights()
        stream = m.weight_stream().copy()                             # synchronises the masters into the module's parameters
        assert np.array_equal(image, pack(m._plan, stream)), step
        for c in ng:
            assert _same(_conv_of(m, c).weight, t._head_masters[c][0]) and _same(_bn_of(m, c).weight, t._head_masters[c][2]) and _same(_bn_of(m, c).bias, t._head_masters[c][3])
            for mine, theirs in ((_bn_of(m, c).running_mean, _bn_of(twin, c).running_mean), (_bn_of(m, c).running_var, _bn_of(twin, c).running_var)):
                assert _same(mine, theirs), (step, c)
        if step in (0, 2):
            m.update_running_stats = False
            y = _forward(m, xd)
            m.update_running_stats = True
            fresh = _mini(tmp_path, "fresh%d" % step)
            fresh.load_state_dict(m.state_dict())
            assert _same(_forward(fresh, xd), y) and np.array_equal(fresh.packed_weights(), image), step
    assert m.active_precision == "f16s3" and not m.overflowed()
    assert losses[1] != losses[0] and np.isfinite(losses).all(), losses
    sd = t.optimizer.state_dict()
    if kind == "adam":
        assert all({"bn_weight", "bn_bias", "exp_avg_bn_weight", "exp_avg_sq_bn_weight", "exp_avg_bn_bias", "exp_avg_sq_bn_bias"} <= set(sd[c]) for c in ng)


@pytest.mark.parametrize("name", ["b_band_k2", "e_slab192", "h_s2"])
def test_probe_step_repacks_every_tile_family(tmp_path, name):
    """One Adam step on a probe whose conv under test runs a bandd tile, a 1x1 slab tile, a generic tile (forced: the first legal id of
    the family): the image equals the host pack of the synchronised parameters, and the next forward that of a fresh model."""
    p = next(q for q in PROBES if q.name == name)
    family = {"b_band_k2": "band", "e_slab192": "slab", "h_s2": "generic"}[name]
    ref, wts, x = setup(p)
    options = dict(p.options, **OPTIONS)

    def build(tag):
        m = _model(tmp_path, p.cfg(), p.H, "f16s3", options, train=True, weights=wts, name=tag)
        m.prepare(p.B, torch.device("cuda", torch.cuda.current_device()))
        n = m._info.n_launches
        launch = launch_of_layer(m.launch_infos(), p.conv_layer)
        v = next(i for i in accepted_ids(_ffi.lib(), m._plan, n, launch, p.B) if i in FAMILIES[family])
        table = [-1] * n
        table[launch] = v
        m.set_tiles(p.B, table)
        return m, launch, v

    m, launch, v = build("m")
    t = T.DarknetTrainer(m, trainable=SCOPE)
    t.min_box_size = 2
    t.optimizer = T.HeadOptimizer("adam", lr=1e-4)
    xd = x.cuda()
    bnd = [torch.from_numpy(im) for im in full_batch(p.H, p.W, 3, p.B)]
    loss = float(t.feed_forward_through_model(xd, bnd))
    assert np.isfinite(loss) and m.launch_infos()[launch].variant == 100 + v and p.conv_layer in [c for c, _ in m.trainable_layers()]
    image = m.packed_weights()
    before = pack(m._plan, wts)
    assert np.array_equal(image, pack(m._plan, m.weight_stream().copy())) and not np.array_equal(image, before)
    y = _forward(m, xd)
    fresh, _, _ = build("fresh")
    fresh.load_state_dict(m.state_dict())
    assert _same(_forward(fresh, xd), y) and np.array_equal(fresh.packed_weights(), image) and not m.overflowed()


# ---------------------------------------------------------------------------------------------- 5., 6. determinism, the optimiser round trip
def test_two_runs_agree_and_a_second_trainer_continues(tmp_path):
    ma, ta, xd, bnd, _ = _trainer(tmp_path, "a")
    mb, tb, _, _, _ = _trainer(tmp_path, "b")
    for t in (ta, tb):
        t.optimizer = T.HeadOptimizer("adam", lr=1e-4)
    ga, gb = ta.batchnorm_gradients(xd, bnd), tb.batchnorm_gradients(xd, bnd)
    assert _same(ga[0], gb[0]) and all(_same(ga[2][k], gb[2][k]) and _same(ga[3][k][0], gb[3][k][0]) and _same(ga[3][k][1], gb[3][k][1]) for k in ga[2])
    la = [float(ta.feed_forward_through_model(xd, bnd)) for _ in range(2)]
    lb = [float(tb.feed_forward_through_model(xd, bnd)) for _ in range(2)]
    assert la == lb and np.array_equal(ma.packed_weights(), mb.packed_weights())
    state = ta.optimizer.state_dict()
    mc, tc, _, _, _ = _trainer(tmp_path, "c")
    tc.optimizer = T.HeadOptimizer("adam", lr=1e-4)
    tc.optimizer.load_state_dict(state)
    l1, l2 = ta.feed_forward_through_model(xd, bnd), tc.feed_forward_through_model(xd, bnd)
    assert _same(l1, l2)
    for layer in state:
        for k in state[layer]:
            if k != "step":
                assert _same(ta.optimizer.state[layer][k], tc.optimizer.state[layer][k]), (layer, k)
        assert ta.optimizer.state[layer]["step"] == tc.optimizer.state[layer]["step"] == 3
    assert np.array_equal(ma.packed_weights(), mc.packed_weights())


# ---------------------------------------------------------------------------------------------- 7. the directional derivative
def test_the_loss_falls_along_the_gradient_by_what_it_says(tmp_path):
    """tests/test_bn_train_gpu.py's check of the same name on the split plan, with its bound: the central difference of the device loss
    along -g (conv weight, gamma and beta of every listed conv moved together through update_conv_bn) against ||g||^2; eps and the allowed
    gap 4 |fd_cpu - dd_cpu| + 2 noise / (2 eps) come from the CPU model (float64 and float32 torch), never from a device result.

    Measured on an MI355X: ||g||^2 1894014.3, eps 3e-07, central difference 1891500.2: gap 2514, allowed 15740."""
    m, t, xd, bnd, images = _trainer(tmp_path)
    _forward(m, xd)
    tenth_heads(m)
    _, _, dws, dbn = t.batchnorm_gradients(xd, bnd)
    l0 = float(t.last_components[0].item())
    g = {c: (dws[c], dbn[c][0], dbn[c][1]) for c in dws}
    p0 = {c: tuple(p.detach().clone() for p in (_conv_of(m, c).weight, _bn_of(m, c).weight, _bn_of(m, c).bias)) for c in g}
    heads = [h for h, _ in m.head_layers()]
    x_in = t._net_input

    def cpu(s, dtype):
        with torch.no_grad():
            val, _, _ = cpu_graph_bn(m, t, dtype, SCOPE, params={c: tuple(p.double() + s * d.cpu().double() for p, d in zip(p0[c], g[c])) for c in g}, x_in=x_in)
        acts = [val[h - 1].detach().numpy() for h in heads]
        ws, bs = [_t64(_conv_of(m, h).weight).numpy() for h in heads], [_t64(_conv_of(m, h).bias).numpy() for h in heads]
        if dtype != torch.float64:
            ws, bs = [a.astype(F) for a in ws], [a.astype(F) for a in bs]
        return cpu_head_model(acts, ws, bs, t.heads, images, 4, None if dtype == torch.float64 else dtype)["loss"]

    g2 = sum(float((d.double() ** 2).sum()) for ds in g.values() for d in ds)
    noise_at = lambda s: abs(cpu(s, torch.float32) - cpu(s, torch.float64))
    noise, eps, gap_cpu = noise_at(0.0), None, None
    for e in (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7):
        fd, dd = (cpu(e, torch.float64) - cpu(-e, torch.float64)) / (2 * e), (cpu(e / 10, torch.float64) - cpu(-e / 10, torch.float64)) / (2 * e / 10)
        if abs(fd - dd) >= 10 * noise / e:
            eps, gap_cpu = e, abs(fd - dd)
    assert eps is not None
    noise = max(noise, noise_at(eps), noise_at(-eps))
    allowed = 4 * gap_cpu + 2 * noise / (2 * eps)

    def loss_at(s):
        for c in g:
            m.update_conv_bn(c, *[p.cuda() + s * d for p, d in zip(p0[c], g[c])])
        t.forward_loss(xd, bnd)
        return float(t.last_components[0].item())
    fd_dev = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
    assert loss_at(0.0) == l0                                         # the parameters are back, bit for bit
    print("split: ||g||^2 device %.8g; eps %.0e; central difference device %.8g; gap %.4g, allowed %.4g (cpu gap %.4g, noise %.4g)" % (
        g2, eps, fd_dev, abs(fd_dev - g2), allowed, gap_cpu, noise))
    assert m.active_precision == "f16s3" and g2 > 0 and abs(fd_dev - g2) <= allowed
