"""GPU tests of training under batch statistics end to end: DarknetTrainer.batchnorm_gradients and feed_forward_through_model on a model
in .train() with options keep_bn_inputs, against torch autograd of the scope's sub-graph with training=True BatchNorm on the CPU.
mini_cfg at 64 x 64, batch 3, scope "backbone"; pool_train_mini_cfg (stem 16), scope "full".  tests/scope_grad_cases.py's recipes with
batch-statistics BatchNorm in place of the folded one, and gamma and beta beside every conv weight.

The mask-flip rule.  A leaky mask comes from the sign of the stored output u = gamma r (z - mu) + beta, r = (var + 1e-5)^-1/2.  The
device's mask may differ from the sign of the float64 model's u only within the forward's own error, carried through the statistics to
first order.  The conv leaves |dz_i| <= E_i = (K + 2) u32 mass_i, mass_i = sum |w| |x| (K = Cin k k fmaf terms and the epilogue's
roundings; u32 = 2^-24).  Then
    d mu  = mean(dz)                                   |d mu|  <= mean(E)
    d var = (2 / N) sum (z_j - mu) dz_j                |d var| <= (2 / N) sum |z_j - mu| E_j          (sum (z_j - mu) = 0 removes d mu)
    d r   = -r^3 d var / 2
    d u_i = gamma r (dz_i - d mu) + gamma (z_i - mu) d r
    |d u_i| <= |gamma| r (E_i + mean(E)) + |gamma| |z_i - mu| r^3 (1 / N) sum |z_j - mu| E_j + 3 u32 (|z_i| |gamma| r + |beta - mu gamma r|)
the last term for the normalise step itself: its two constants rounded to float once each, one fma.  Every quantity is evaluated in
float64 on the CPU from the float64 model's z and x (flip_bound), never from a device result; float32 torch's own flips against the
float64 model are first held to the same bound."""
import numpy as np
import pytest
import torch

from block_grad_cases import opt_update_f32
from full_grad_cases import full_batch, pool_winners
from head_grad_cases import cpu_head_model, pack
from loss_cases import bits
from scope_grad_cases import KEEP, U, _bn_of, _conv_of, _forward, _frames, _model, _same, _t64, tenth_heads, torch_pool
from realtimeobjectdetection_amd import cfgs, train as T

pytestmark = pytest.mark.gpu
F = np.float32
fn = torch.nn.functional
B = 3
CASES = {"mini-backbone": (lambda: cfgs.mini_cfg(64, 64), "backbone", 80), "pool-full": (lambda: cfgs.pool_train_mini_cfg(64, 64, classes=3, stem=16), "full", 3)}


def _trainer(tmp_path, case, name="m", running=False, options=None):
    text, scope, classes = CASES[case]
    m = _model(tmp_path, text(), 64, "fp32", dict(KEEP[scope], keep_bn_inputs=1) if options is None else options, train=True, name=name)
    m.update_running_stats = running
    t = T.DarknetTrainer(m, trainable=scope)
    t.min_box_size = 4
    xd = _frames(B, 64, None)
    images = full_batch(64, 64, classes, B)
    return m, t, scope, xd, [torch.from_numpy(im) for im in images], images


# ---------------------------------------------------------------------------------------------- the CPU model of the scope's sub-graph
def cpu_graph_bn(m, t, dtype, scope, params=None, masks=None, x_in=None, winners=None):
    """scope_grad_cases.cpu_graph with training=True BatchNorm: every BatchNorm conv of the graph is conv2d -> F.batch_norm(z, None, None,
    gamma, beta, True, 0.0, 1e-5) -> leaky (a product with the DEVICE's ``masks[layer]`` where given, else torch's leaky_relu), with
    conv weight, gamma and beta as leaves (``params``: {conv: (W, gamma, beta)} in place of the module's).  Returns (values per layer,
    {conv: (W, gamma, beta)}, {conv: (u, x, z)})."""
    layers, readers, member, scales = t._graph(scope)
    cast = lambda a: torch.as_tensor(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).to(dtype)
    val, leaves, pres = ({} if x_in is None else {-1: cast(x_in)}), {}, {}

    def value(src):
        if src not in val:
            assert not member[src]
            val[src] = cast(m.read_layer(src, B))
        return val[src]

    for L in layers:
        i = L.index
        if not member[i]:
            continue
        if L.type == "convolutional":
            conv, x = _conv_of(m, i), value(i - 1)
            if i in scales:
                bn = _bn_of(m, i)
                W, g, b = (cast(p).requires_grad_(True) for p in ((conv.weight, bn.weight, bn.bias) if params is None or i not in params else params[i]))
                leaves[i] = (W, g, b)
                z = fn.conv2d(x, W, stride=L.stride, padding=L.size // 2)
                u = fn.batch_norm(z, None, None, g, b, True, 0.0, 1e-5)
                pres[i] = (u, x, z)
                val[i] = u if not L.leaky else u * cast(masks[i]) if masks is not None else fn.leaky_relu(u, 0.1)
            else:
                val[i] = fn.conv2d(x, cast(conv.weight), cast(conv.bias))
        elif L.type == "maxpool":
            x = value(i - 1)
            if winners is None:
                val[i] = torch_pool(x, L.stride)
            else:
                idx = torch.from_numpy(winners[i])
                val[i] = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
        elif L.type == "upsample":
            val[i] = fn.interpolate(value(i - 1), scale_factor=2, mode="nearest") if L.nearest else fn.interpolate(value(i - 1), scale_factor=2, mode="bilinear", align_corners=False)
        elif L.type == "shortcut":
            val[i] = value(L.srcs[0]) + value(L.srcs[1])
        else:
            parts, off = [], 0
            for s in L.srcs:
                parts.append(value(s) if member[s] else cast(m.read_layer(i, B))[:, off:off + layers[s].cout])
                off += layers[s].cout
            val[i] = torch.cat(parts, 1)
    return val, leaves, pres


def cpu_grads_bn(m, t, dtype, scope, masks, dzs, x_in, winners):
    val, leaves, pres = cpu_graph_bn(m, t, dtype, scope, masks=masks, x_in=x_in, winners=winners)
    sum((val[head] * dz.detach().cpu().to(dtype)).sum() for (head, _), dz in zip(m.head_layers(), dzs)).backward()
    return {i: tuple(p.grad.numpy().astype(np.float64) for p in ps) for i, ps in leaves.items()}, pres


def flip_bound(L, W, gamma, beta, x, z):
    """|d u| of the module docstring, float64 numpy [B,C,H,W], from float64 tensors of the CPU model."""
    W, gamma, beta, x, z = (a.detach().double() for a in (W, gamma, beta, x, z))
    E = ((W.shape[1] * L.size * L.size + 2) * U * fn.conv2d(x.abs(), W.abs(), stride=L.stride, padding=L.size // 2)).numpy()
    z, g, b = z.numpy(), np.abs(gamma.numpy()).reshape(1, -1, 1, 1), beta.numpy().reshape(1, -1, 1, 1)
    ax = (0, 2, 3)
    mu, var = z.mean(axis=ax, keepdims=True), z.var(axis=ax, keepdims=True)
    r, d = 1.0 / np.sqrt(var + 1e-5), np.abs(z - mu)
    own = 3 * U * (np.abs(z) * g * r + np.abs(b - mu * gamma.numpy().reshape(1, -1, 1, 1) * r))
    return g * r * (E + E.mean(axis=ax, keepdims=True)) + g * d * r ** 3 * (d * E).mean(axis=ax, keepdims=True) + own


# ---------------------------------------------------------------------------------------------- 1, 2. gradients, masks
@pytest.mark.parametrize("case", sorted(CASES))
def test_batchnorm_gradients_against_autograd(tmp_path, case):
    """dW, dgamma and dbeta of DarknetTrainer.batchnorm_gradients for every listed conv against torch autograd of the sub-graph with
    training=True BatchNorm, the DEVICE's leaky masks and pool winners, pulled back from the device's dz: once in float64 (the truth),
    once in float32 torch (the floor).  The gate, per conv and per parameter: rms and max of (device - float64) / max |float64| are at
    most 4 x the same figures of (float32 - float64).  The masks: the rule of the module docstring, float32 torch's own flips first.
    The three-tuple entries are batchnorm_gradients without its last element, bit for bit, and a second call repeats every bit.

    Measured on an MI355X, worst rms ratio / worst max ratio over all convs and the three parameters (no mask flipped anywhere):
      mini-backbone (14 convs)  1.03 / 1.53        pool-full (9 convs)  1.14 / 1.49"""
    m, t, scope, xd, bnd, _ = _trainer(tmp_path, case)
    _forward(m, xd)
    tenth_heads(m)
    loss, head_grads, grads, bn_grads = t.batchnorm_gradients(xd, bnd)
    listed = [c for c, _ in (m.trainable_layers() if scope == "backbone" else m.full_layers())]
    assert m.active_precision == "fp32" and int(t.status.item()) == 0 and listed and sorted(grads) == sorted(bn_grads) == listed
    loss2, heads2, again = t.gradients(xd, bnd)
    assert _same(loss, loss2) and all(_same(grads[k], again[k]) for k in grads) and all(_same(head_grads[k][0], heads2[k][0]) for k in heads2)
    _, _, _, bn_again = t.batchnorm_gradients(xd, bnd)
    assert all(_same(bn_grads[k][0], bn_again[k][0]) and _same(bn_grads[k][1], bn_again[k][1]) for k in bn_grads)
    layers, readers, member, scales = t._graph(scope)
    assert all(s is None for s in scales.values())                    # batch mode: no frozen scale anywhere
    pools = [L.index for L in layers if L.type == "maxpool" and member[L.index]]
    masks = {c: np.where(m.read_layer(c, B).cpu().numpy() > 0, 1.0, 0.1) for c in listed if layers[c].leaky}
    winners = {p: pool_winners(m.read_layer(p - 1, B).cpu().numpy(), layers[p].stride) for p in pools}
    dzs = T.yolo_loss_grad_async(t._forward_train(xd), bnd, t.heads, t.num_classes, t.min_box_size)["grad_raw"]
    x_in = t._net_input
    want, pres = cpu_grads_bn(m, t, torch.float64, scope, masks, dzs, x_in, winners)
    floor, _ = cpu_grads_bn(m, t, torch.float32, scope, masks, dzs, x_in, winners)
    over = []
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    for c in listed:
        L = layers[c]
        u, x, z = (a.detach() for a in pres[c])
        # float32 torch first, on the CPU alone: the same conv and BatchNorm in float32 on the float64 model's input obey the bound
        W64, g64, b64 = (_t64(p) for p in (_conv_of(m, c).weight, _bn_of(m, c).weight, _bn_of(m, c).bias))
        u32 = fn.batch_norm(fn.conv2d(x.float(), W64.float(), stride=L.stride, padding=L.size // 2), None, None, g64.float(), b64.float(), True, 0.0, 1e-5).numpy()
        flips32 = (u32 > 0) != (u.numpy() > 0)
        assert (np.abs(u.numpy())[flips32] <= flip_bound(L, W64, g64, b64, x, z)[flips32]).all(), (case, c, "float32 torch", int(flips32.sum()))
        bound = flip_bound(L, *[torch.as_tensor(p) for p in (_conv_of(m, c).weight, _bn_of(m, c).weight, _bn_of(m, c).bias)], x, z)
        flips = (u.numpy() > 0) != (m.read_layer(c, B).cpu().numpy() > 0)
        assert (np.abs(u.numpy())[flips] <= bound[flips]).all(), (case, c, int(flips.sum()))
        got = (grads[c], bn_grads[c][0], bn_grads[c][1])
        for name, g, w, f in zip(("dW", "dgamma", "dbeta"), got, want[c], floor[c]):
            g, ref = g.cpu().numpy().astype(np.float64), np.abs(w).max()
            assert g.shape == w.shape and ref > 0, (case, c, name)
            e_dev, e_32 = (g - w) / ref, (f - w) / ref
            print("%s conv %d %s (%d flips, float32 torch %d): rms %.3g (floor %.3g, ratio %.2f)  max %.3g (floor %.3g, ratio %.2f)" % (
                case, c, name, int(flips.sum()), int(flips32.sum()), rms(e_dev), rms(e_32), rms(e_dev) / rms(e_32), np.abs(e_dev).max(), np.abs(e_32).max(),
                np.abs(e_dev).max() / np.abs(e_32).max()))
            if not (rms(e_dev) <= 4 * rms(e_32) and np.abs(e_dev).max() <= 4 * np.abs(e_32).max()):
                over.append((c, name, round(rms(e_dev) / rms(e_32), 2), round(float(np.abs(e_dev).max() / np.abs(e_32).max()), 2)))
    assert not over, (case, "(conv, parameter, rms ratio, max ratio) over 4 x the float32 floor", over)


# ---------------------------------------------------------------------------------------------- 3. the directional derivative
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_loss_falls_along_the_gradient_by_what_it_says(tmp_path, case):
    """scope_grad_cases.check_directional_derivative's recipe with conv weight, gamma and beta of every listed conv moved together through
    update_conv_bn: the central difference of the device loss along -g against ||g||^2 over all three kinds of parameter; eps and the
    allowed gap from the CPU model (torch's own leaky_relu and pools, training=True BatchNorm), never from a device result."""
    m, t, scope, xd, bnd, images = _trainer(tmp_path, case)
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
            val, _, _ = cpu_graph_bn(m, t, dtype, scope, params={c: tuple(p.double() + s * d.cpu().double() for p, d in zip(p0[c], g[c])) for c in g}, x_in=x_in)
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
    print("%s: ||g||^2 device %.8g; eps %.0e; central difference device %.8g; gap %.4g, allowed %.4g (cpu gap %.4g, noise %.4g)" % (
        case, g2, eps, fd_dev, abs(fd_dev - g2), allowed, gap_cpu, noise))
    assert g2 > 0 and abs(fd_dev - g2) <= allowed


# ---------------------------------------------------------------------------------------------- 4. the training step
@pytest.mark.parametrize("case", sorted(CASES))
def test_training_steps_under_batch_statistics(tmp_path, case):
    """feed_forward_through_model in batch mode, an SGD step and then two Adam steps (lr 1e-4).  After each: the masters and moments of
    conv weight, gamma and beta (and of the heads' weight and bias) equal block_grad_cases.opt_update_f32 of the gradients
    batchnorm_gradients returned for the state before the step, bit for bit; the packed image equals the host pack of the synchronised
    parameters, bit for bit, and bn.weight / bn.bias equal their masters; running_mean and running_var equal what the forward alone
    leaves (a twin model that only runs the forwards, from the same buffers); the loss changes and stays finite."""
    m, t, scope, xd, bnd, _ = _trainer(tmp_path, case, running=True)
    twin = _trainer(tmp_path, case, name="twin", running=True)[0]
    host = lambda a: None if a is None else a.detach().cpu().numpy()
    names = (("weight", ""), ("bias", "_bias"), ("bn_weight", "_bn_weight"), ("bn_bias", "_bn_bias"))
    losses = []
    for step, kind in enumerate(["sgd", "adam", "adam"]):
        if step < 2:
            t.optimizer = T.HeadOptimizer(kind, lr=1e-4)
        m.update_running_stats = False                                # (the gradients below are a look, not a step of the reference)
        _, hg, ng, bg = t.batchnorm_gradients(xd, bnd)
        m.update_running_stats = True
        grads = {k: (host(dw), host(db), None, None) for k, (dw, db) in hg.items()}
        grads.update({k: (host(dw), None, host(bg[k][0]), host(bg[k][1])) for k, dw in ng.items()})
        masters = t._masters(list(hg) + list(ng), xd.device)
        before = {k: tuple(host(p) for p in (list(masters[k]) + [None, None])[:4]) for k in grads}
        state = {k: {n: host(v) for n, v in t.optimizer.state.get(k, {}).items() if n.startswith("exp_avg")} for k in grads}
        rs = {c: (host(_bn_of(m, c).running_mean).copy(), host(_bn_of(m, c).running_var).copy()) for c in ng}
        assert all(np.array_equal(bits(rs[c][0]), bits(host(_bn_of(twin, c).running_mean))) for c in ng)
        if step:                                                      # the twin runs the stepped parameters, and only forwards
            for c in ng:
                twin.update_conv_bn(c, *[torch.from_numpy(p) for p in (before[c][0], before[c][2], before[c][3])])
            for h_, _ in hg.items():
                twin.update_conv(h_, torch.from_numpy(before[h_][0]), torch.from_numpy(before[h_][1]))
        losses.append(float(t.feed_forward_through_model(xd, bnd)))
        with twin.train_mode():
            _forward(twin, xd)
        for k in grads:
            st = t.optimizer.state[k]
            assert st["step"] == (1 if step < 2 else 2) and st["weight"] is t._head_masters[k][0]
            for which, (name, sfx) in enumerate(names):
                if before[k][which] is None:
                    assert name not in st
                    continue
                zero = np.zeros_like(before[k][which])
                w1, m1, v1 = opt_update_f32(kind, before[k][which], grads[k][which], state[k].get("exp_avg" + sfx, zero), state[k].get("exp_avg_sq" + sfx, zero),
                                            1e-4, step=st["step"])
                assert np.array_equal(bits(host(st[name])), bits(w1)), (step, k, name)
                if kind == "adam":
                    assert np.array_equal(bits(host(st["exp_avg" + sfx])), bits(m1)) and np.array_equal(bits(host(st["exp_avg_sq" + sfx])), bits(v1)), (step, k, name)
        image = m.packed_weights()
        stream = m.weight_stream().copy()                             # synchronises the masters into the module's parameters
        assert np.array_equal(image, pack(m._plan, stream)), step
        for c in ng:
            assert _same(_conv_of(m, c).weight, t._head_masters[c][0]) and _same(_bn_of(m, c).weight, t._head_masters[c][2]) and _same(_bn_of(m, c).bias, t._head_masters[c][3])
            for mine, theirs in ((_bn_of(m, c).running_mean, _bn_of(twin, c).running_mean), (_bn_of(m, c).running_var, _bn_of(twin, c).running_var)):
                assert _same(mine, theirs), (step, c)
            assert not np.array_equal(bits(host(_bn_of(m, c).running_mean)), bits(rs[c][0])), (step, c)
    sd = t.optimizer.state_dict()
    assert all({"bn_weight", "bn_bias", "exp_avg_bn_weight", "exp_avg_sq_bn_weight", "exp_avg_bn_bias", "exp_avg_sq_bn_bias"} <= set(sd[c]) for c in ng)
    assert losses[1] != losses[0] and np.isfinite(losses).all(), losses


# ---------------------------------------------------------------------------------------------- 6. the misconfiguration
def test_a_training_mode_model_without_the_option_is_refused_by_name(tmp_path):
    text, scope, _ = CASES["mini-backbone"]
    m = _model(tmp_path, text(), 64, "fp32", KEEP[scope], train=True)
    with pytest.raises(RuntimeError, match="keep_bn_inputs"):
        T.DarknetTrainer(m, trainable="backbone")
    t = T.DarknetTrainer(m)                                           # heads alone: nothing behind them is trained, nothing is asked
    with pytest.raises(RuntimeError, match="keep_bn_inputs"):
        t.gradients(_frames(B, 64, None), [None] * B, scope="backbone")
    m.eval()                                                          # an eval model is untouched
    assert T.DarknetTrainer(m, trainable="backbone").trainable == "backbone"
