"""GPU tests of the device optimiser step of the detection heads (csrc/head_step.hip through rtod_plan_step_conv,
Darknet.step_conv, HeadOptimizer and DarknetTrainer.feed_forward_through_model): the device pack against the host pack bit for
bit, device SGD against head_step bit for bit, device Adam against torch's own optimiser (tests/golden/adam_step.npz), stream
capture, five Adam steps against a float64 CPU model of the heads, and the rule that stale module parameters are never packed.

Gates.
* Pack, SGD, capture, state round trip: identical bits, whole arrays and the whole packed image as uint32 words.
* Adam against the fixture: tests/head_opt_cases.py (D_w, D_m, D_v; max and rms within 4 x the recorded float32 floor of torch's own
  float32 optimiser; D = 0 exact).
* Five steps: the docstring of test_five_adam_steps_follow_the_float64_model.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_opt_cases as A
from head_grad_cases import conv_stream_ranges, cpu_head_model, pack
from loss_cases import bits
from test_head_grad_gpu import _conv_of, _forward, _head_state, _model, _trainer, step_batch
from realtimeobjectdetection_amd import _ffi, cfgs, synth
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text
from realtimeobjectdetection_amd.train import HeadOptimizer

pytestmark = pytest.mark.gpu
F = np.float32
HEADS = ((14, 255, 1024), (22, 255, 512))                            # mini_cfg(64, 64): conv layer, Cout, Cin


@pytest.fixture(scope="module")
def adam_cases(golden_dir):
    return A.load_adam_cases(golden_dir)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))


def _batch():
    x, images = step_batch()
    return torch.from_numpy(x).cuda(), [torch.from_numpy(im) for im in images]


# ------------------------------------------------------------------------------------------ 1. the device pack is the host pack
@pytest.mark.parametrize("precision,train", [("fp32", False), ("f16s3", False), ("f16", False), ("f16s3", True)])
def test_device_pack_is_the_host_pack_bit_for_bit(tmp_path, precision, train):
    """SGD with lr = 0 leaves the masters as they are and re-packs them.  dW is random and finite, of either sign, except where a
    master is -0: there it is made non-negative, since IEEE gives (-0) - (-0) = +0 — for the documented w - fl(lr * g) as for torch's
    w.sub_(g * lr) — and the test is about the pack, not about that sign."""
    res, B = 64, 2
    text = cfgs.mini_cfg(res, res)
    options = {"bn_batch_split": 1} if train else {}
    m = _model(tmp_path, text, res, precision, options, train)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=3)).cuda()
    before = _forward(m, x)
    assert m.active_precision == precision and m.head_layers() == [(14, 13), (22, 21)]
    stream = m.weight_stream().copy()
    ranges = conv_stream_ranges(build_ir(parse_cfg_text(text), res))
    rng = np.random.default_rng(31)
    opt = _ffi.OptStep(0, 0.0, 0, 0, 0, 0)
    for k, (layer, cout, cin) in enumerate(HEADS):
        w, b = A.adversarial_head(cout, cin, 100 + k)
        assert np.signbit(w[w == 0]).any() and not w[0].any() and np.abs(w[3]).max() == F(2.0 ** -45) and np.abs(w[4]).max() == F(2.0 ** 30)
        dw, db = (rng.standard_normal(w.shape) * 10.0 ** rng.uniform(-3, 3, w.shape)).astype(F), rng.standard_normal(cout).astype(F)
        dw[np.signbit(w) & (w == 0)] = np.abs(dw[np.signbit(w) & (w == 0)])
        db[np.signbit(b) & (b == 0)] = np.abs(db[np.signbit(b) & (b == 0)])
        wd, bd = _dev(w).view(cout, cin, 1, 1), _dev(b)
        m.step_conv(layer, opt, wd, bd, _dev(dw).view(cout, cin, 1, 1), _dev(db))
        assert np.array_equal(bits(wd.cpu().numpy().reshape(cout, cin)), bits(w)) and np.array_equal(bits(bd.cpu().numpy()), bits(b)), layer
        off, n, bn = ranges[layer]
        assert not bn and n == cout + cout * cin
        stream[off:off + cout] = b
        stream[off + cout:off + n] = w.reshape(-1)
    image = m.packed_weights()
    want = pack(m._plan, stream)
    assert image.dtype == np.uint32 and image.shape == want.shape
    diff = np.flatnonzero(image != want)
    assert diff.size == 0, (precision, train, diff[:8].tolist(), diff.size)          # the whole image: other convs, padding channels, padding K
    assert np.array_equal(bits(m.weight_stream()), bits(stream))                       # ... and the stream picks the masters up
    after = _forward(m, x)
    fresh = _model(tmp_path, text, res, precision, options, train, weights=stream, name="fresh")
    assert np.array_equal(bits(after.cpu().numpy()), bits(_forward(fresh, x).cpu().numpy())) and not _same(after, before)
    assert np.array_equal(fresh.packed_weights(), image)


# ------------------------------------------------------------------------------------------ 2. device SGD is head_step
@pytest.mark.parametrize("precision", ["fp32", "f16s3"])
def test_device_sgd_is_head_step_bit_for_bit(tmp_path, precision):
    xd, bnd = _batch()
    ma, ta = _trainer(tmp_path, precision)
    mb, tb = _trainer(tmp_path, precision)
    tb.optimizer = HeadOptimizer("sgd", lr=1e-4)
    la = [ta.head_step(xd, bnd, 1e-4) for _ in range(3)]
    lb = [tb.feed_forward_through_model(xd, bnd) for _ in range(3)]
    assert ma.active_precision == mb.active_precision == precision
    assert all(_same(a, b) and a.dim() == 0 and a.is_cuda for a, b in zip(la, lb)), ([float(a) for a in la], [float(b) for b in lb])
    assert float(lb[0]) > float(lb[1]) > float(lb[2])
    for layer, _, _ in HEADS:
        assert _same(ta._head_masters[layer][0], tb._head_masters[layer][0]) and _same(ta._head_masters[layer][1], tb._head_masters[layer][1]), layer
        assert not _same(_conv_of(mb, layer).weight, tb._head_masters[layer][0])       # the module's parameters lag behind ...
    version = (mb._weights_version, mb._plan_weights_version)
    tb.sync_parameters()
    assert (mb._weights_version, mb._plan_weights_version) == version                  # ... until asked for; no re-pack follows
    for layer, _, _ in HEADS:
        assert _same(_conv_of(mb, layer).weight, _conv_of(ma, layer).weight) and _same(_conv_of(mb, layer).bias, _conv_of(ma, layer).bias), layer
    assert np.array_equal(ma.packed_weights(), mb.packed_weights())
    # the two paths mix: one more of each on both, in opposite orders of construction
    l1, l2 = ta.feed_forward_through_model(xd, bnd), tb.head_step(xd, bnd, 1e-2)
    assert _same(l1, l2)


# ------------------------------------------------------------------------------------------ 3. Adam against the fixture
def _adam_call(m, c, bias_col=0):
    w, g, mm, v = (_dev(a) for a in c["inputs"])
    b, db, mb, vb = (_dev(a[:, bias_col].copy()) for a in c["inputs"])
    cout, cin = A.SHAPE
    opt = _ffi.OptStep(1, A.LR, A.BETAS[0], A.BETAS[1], A.EPS, c["t"])
    m.step_conv(22, opt, w.view(cout, cin, 1, 1), b, g.view(cout, cin, 1, 1), db, (mm.view(cout, cin, 1, 1), v.view(cout, cin, 1, 1), mb, vb))
    return [t.cpu().numpy() for t in (w, mm, v, b, mb, vb)], m.packed_weights()


def test_adam_against_torchs_optimiser(tmp_path, adam_cases):
    m = _model(tmp_path, cfgs.mini_cfg(64, 64), 64, "fp32")
    _forward(m, torch.from_numpy(synth.synth_frames(1, 64, seed=3)).cuda())
    for c in adam_cases:
        got, image = _adam_call(m, c)
        for k, n in enumerate("wmv"):
            mx, rms, exact = A.errors(got[k], c["ref"][k], c["d"][k])
            fmx, frms = c["floor"][n]
            print("t = %d %s: max %.3g (floor %.3g, x %.2f)  rms %.3g (floor %.3g, x %.2f)" % (c["t"], n, mx, fmx, mx / fmx, rms, frms, rms / frms))
            assert exact, (c["t"], n)                                                  # D = 0: exact
            assert mx <= 4 * fmx and rms <= 4 * frms, (c["t"], n, mx, rms, fmx, frms)
            # the bias takes the same step: column 0 of the arrays went in as the bias vector
            assert np.array_equal(bits(got[3 + k]), bits(np.ascontiguousarray(got[k][:, 0]))), (c["t"], n)
        again, image2 = _adam_call(m, c)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again)) and np.array_equal(image, image2), c["t"]


# ------------------------------------------------------------------------------------------ 4. stream capture
def test_adam_step_under_stream_capture(tmp_path, adam_cases):
    m = _model(tmp_path, cfgs.mini_cfg(64, 64), 64, "f16s3")
    _forward(m, torch.from_numpy(synth.synth_frames(1, 64, seed=3)).cuda())
    c = adam_cases[2]
    cout, cin = A.SHAPE
    start = [_dev(a).view(cout, cin, 1, 1) for a in c["inputs"]] + [_dev(a[:, 1].copy()) for a in c["inputs"]]   # w, g, m, v, then the bias's
    w, g, mm, v, b, db, mb, vb = [t.clone() for t in start]
    state = (w, g, mm, v, b, db, mb, vb)
    opt = _ffi.OptStep(1, A.LR, A.BETAS[0], A.BETAS[1], A.EPS, c["t"])
    call = lambda: m.step_conv(22, opt, w, b, g, db, (mm, v, mb, vb))

    def restore():
        for t, s in zip(state, start):
            t.copy_(s)
    dev = w.device
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                     # warm-up on a non-default stream, as capture requires
        call()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # a synchronisation or an allocation inside the call would fail here
        call()
    restore()
    graph.replay()
    torch.cuda.synchronize(dev)
    replayed, image = [t.clone() for t in state], m.packed_weights()
    assert not _same(replayed[0], start[0]) and not _same(replayed[2], start[2])
    restore()
    call()
    assert all(_same(a, b) for a, b in zip(state, replayed)) and np.array_equal(m.packed_weights(), image)


# ------------------------------------------------------------------------------------------ 5. end to end
LR5 = 1e-2


def _cpu_trajectory(xs, ws, bs, heads, images, dtype, lr, steps):
    """Losses before each of ``steps`` torch.optim.Adam steps on the heads and after the last, on the CPU in ``dtype``."""
    dt = torch.float64 if dtype is None else dtype
    cast = (lambda a: a) if dtype is None else (lambda a: a.astype(F))
    params = [torch.nn.Parameter(torch.tensor(np.asarray(a), dtype=dt)) for a in list(ws) + list(bs)]
    opt = torch.optim.Adam(params, lr=lr)
    xs = [cast(a) for a in xs]
    losses = []
    for k in range(steps + 1):
        r = cpu_head_model(xs, [p.detach().numpy() for p in params[:len(ws)]], [p.detach().numpy() for p in params[len(ws):]], heads, images, 4, dtype)
        losses.append(r["loss"])
        if k < steps:
            for p, gr in zip(params, r["dw"] + r["db"]):
                p.grad = torch.tensor(gr, dtype=dt)
            opt.step()
    return losses


def test_five_adam_steps_follow_the_float64_model(tmp_path):
    """Five feed_forward_through_model calls with the default optimiser (Adam, the reference's) on the batch of step_batch, fp32
    plan, min_box_size = 4.

    lr was chosen while writing the test from a float64 CPU model of the heads (head_grad_cases.cpu_head_model plus
    torch.optim.Adam in float64 on the CPU oracle's head inputs for this batch; the backbone is frozen and in eval mode, so the
    head inputs do not change between steps), run without a device: the largest of 1e-2, 3e-3, 1e-3, ... at which the modelled
    loss falls at every one of the five steps.  That is 1e-2, the reference's own lr, where the model goes
        709.77 -> 212.48 -> 211.04 -> 190.69 -> 98.03 -> 61.32
    (3e-3: 709.77 -> 412.29 -> 234.20 -> 147.39 -> 118.34 -> 112.04).  The same model in float32 differs from it by 4.4e-5, 6.6e-6,
    3.4e-5, 1.1e-5, 4.2e-5, 2.5e-5 at the six evaluations.

    On the device both trajectories are recomputed from the device's own head inputs (read_layer).  The device loss (the double of
    last_components) must fall at every step and differ from the float64 trajectory at evaluation k by at most
        4 * |float32 CPU - float64 CPU| at k   +   noise,      noise = |L_cpu,float32 - L_cpu,float64| at the first evaluation,
    the one-evaluation loss noise of test_the_step_descends_by_what_the_gradient_says.  Neither number was adjusted to a device
    result."""
    B, steps = 3, 5
    m, t = _trainer(tmp_path, "fp32")
    assert t.optimizer.kind == "adam"
    t.optimizer.lr = LR5
    xd, bnd = _batch()
    _, images = step_batch()
    t.forward_loss(xd, bnd)                                           # the head inputs and weights before the first step
    xs, ws, bs = _head_state(m, B)
    dev_losses = []
    for _ in range(steps):
        loss = t.feed_forward_through_model(xd, bnd)
        assert loss.dim() == 0 and loss.is_cuda
        dev_losses.append(float(t.last_components[0].item()))
        assert float(loss) == float(F(dev_losses[-1]))
    t.forward_loss(xd, bnd)
    dev_losses.append(float(t.last_components[0].item()))
    assert int(t.status.item()) == 0
    l64 = _cpu_trajectory(xs, ws, bs, t.heads, images, None, LR5, steps)
    l32 = _cpu_trajectory(xs, ws, bs, t.heads, images, torch.float32, LR5, steps)
    noise = abs(l32[0] - l64[0])
    allowed = [4 * abs(a - b) + noise for a, b in zip(l32, l64)]
    gaps = [abs(a - b) for a, b in zip(dev_losses, l64)]
    print("device  ", ["%.9g" % v for v in dev_losses])
    print("float64 ", ["%.9g" % v for v in l64])
    print("float32 ", ["%.9g" % v for v in l32])
    print("gaps    ", ["%.3g" % v for v in gaps], "allowed", ["%.3g" % v for v in allowed])
    assert all(a > b for a, b in zip(l64, l64[1:])), l64              # the model falls at this lr on the device's inputs too
    assert all(a > b for a, b in zip(dev_losses, dev_losses[1:])), dev_losses
    assert all(g <= a for g, a in zip(gaps, allowed)), (gaps, allowed)
    assert {k: st["step"] for k, st in t.optimizer.state.items()} == {14: steps, 22: steps}


# ------------------------------------------------------------------------------------------ 6. stale parameters are never packed
def test_stale_parameters_are_never_packed(tmp_path):
    xd, bnd = _batch()
    m, t = _trainer(tmp_path, "f16s3")
    t.optimizer.lr = 1e-3
    start = m.weight_stream().copy()
    for _ in range(3):
        t.feed_forward_through_model(xd, bnd)
    saved = t.optimizer.state_dict()
    assert sorted(saved) == [14, 22] and sorted(saved[14]) == ["bias", "exp_avg", "exp_avg_bias", "exp_avg_sq", "exp_avg_sq_bias", "step", "weight"]
    assert saved[14]["step"] == 3 and saved[14]["weight"] is t._head_masters[14][0]
    assert not _same(_conv_of(m, 14).weight, t._head_masters[14][0])                   # stale here
    m.precision = "fp32"                                              # a new plan: packs from the parameters
    y = _forward(m, xd)
    assert m.active_precision == "fp32"
    t.sync_parameters()
    stream = m.weight_stream()
    fresh = _model(tmp_path, cfgs.mini_cfg(64, 64), 64, "fp32", {"keep_head_inputs": 1}, weights=stream, name="fresh")
    assert np.array_equal(bits(y.cpu().numpy()), bits(_forward(fresh, xd).cpu().numpy()))
    ranges = conv_stream_ranges(build_ir(parse_cfg_text(cfgs.mini_cfg(64, 64)), 64))
    changed = np.zeros(stream.size, bool)
    for layer, _, _ in HEADS:
        off, n, _ = ranges[layer]
        changed[off:off + n] = True
        # the training is in the stream: every channel of an anchor that owns an object, the objectness channels of the others
        assert (bits(stream[off:off + n]) != bits(start[off:off + n])).mean() > 3 / 255, layer
        assert np.array_equal(bits(stream[off + 255:off + n]), bits(t._head_masters[layer][0].cpu().numpy().reshape(-1))), layer
    assert np.array_equal(bits(stream[~changed]), bits(start[~changed]))               # ... in the head blocks only
    # state_dict() and invalidate_weights() see the masters too
    m.precision = "f16s3"
    _forward(m, xd)
    t.feed_forward_through_model(xd, bnd)
    sd = m.state_dict()
    assert _same(sd["module_list.14.conv_14.weight"], t._head_masters[14][0]) and _same(sd["module_list.22.conv_22.bias"], t._head_masters[22][1])
    t.feed_forward_through_model(xd, bnd)
    m.invalidate_weights()
    assert _same(_conv_of(m, 22).weight, t._head_masters[22][0])
    # a second trainer continues from the optimiser's state
    state = t.optimizer.state_dict()
    assert state[14]["step"] == 5
    m2, t2 = _trainer(tmp_path, "f16s3")
    t2.optimizer.lr = 1e-3
    t2.optimizer.load_state_dict(state)
    assert t2.optimizer.state[14]["weight"] is not state[14]["weight"] and t2._head_masters[14][0] is t2.optimizer.state[14]["weight"]
    la, lb = t.feed_forward_through_model(xd, bnd), t2.feed_forward_through_model(xd, bnd)
    assert _same(la, lb)
    for layer, _, _ in HEADS:
        for k in ("weight", "bias", "exp_avg", "exp_avg_sq", "exp_avg_bias", "exp_avg_sq_bias"):
            assert _same(t.optimizer.state[layer][k], t2.optimizer.state[layer][k]), (layer, k)
        assert t.optimizer.state[layer]["step"] == t2.optimizer.state[layer]["step"] == 6
    assert np.array_equal(m.packed_weights(), m2.packed_weights())
