"""GPU tests of batch-statistics BatchNorm on the split-f16 kernels (Darknet.options = {"bn_batch_split": 1}, module in training
mode, precision "f16s3" / "auto").  Run on an MI355X with ``pytest -m gpu``.

1. Layer-local float64 model (tests/bn_split_model.py) on every square probe and on mini_cfg at 64x64 (B = 2, 3): every stored
   BatchNorm layer is recomputed from the GPU's OWN stored input and shortcut operand; r = (value - model) / D must stay within
   GATE_M = 4 times the floors of three float32 evaluations of the same layer (f16s3_emulation.gate; the CPU test
   tests/test_bn_split_host.py shows that this gate catches three planted defects).
2. Every tile id rtod_plan_set_tiles accepts for a probe's conv under test gives the layer's bits: stored layers, output and
   the batch statistics of every BatchNorm layer (rtod_plan_bn_batch_stats) bit-identical to the default tile's; a second
   forward and a HIP-graph replay repeat them.
3. End to end against the real reference run in training mode (tests/golden/trainbn.npz), precision "auto": the split path
   and the exact-fp32 batch-statistics path measured in the same test against the same golden rows.

   MEASURED (MI355X; rel_err against the golden rows, p99.9 / max):
       yolov3_416_b2   split 5.56e-05 / 1.33e-04    fp32 batch-BN 5.76e-05 / 2.00e-04
       yolov3_320_b3   split 5.41e-05 / 1.52e-04    fp32 batch-BN 5.61e-05 / 2.37e-04
   The split path holds the mode's documented gate (p99.9 <= 1e-4, max <= 3.5e-4: test_gpu_parity.py,
   test_training_mode_batch_statistics_vs_reference_golden), so that gate is what is asserted.
4. YOLOv3-tiny (a BatchNorm conv with 16 input channels) with the option and "auto" falls back to the exact-fp32 path.

Every test prints its figures ("GATE ..." / "E2E ..." lines).
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from oracle import darknet_ref as O
from bn_split_model import BY_NAME, SQUARE, bn_layer_model, bn_layers
from conv_probes import FAMILIES, accepted_ids, launch_of_layer, legal_ids, setup
from f16s3_emulation import floors, gate, residual, rms_max
from test_gpu_parity import rel_err
from test_oracle_golden import NETS

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = [p.name for p in SQUARE]


def _model(cfg_text, res, d, wts, options=(), precision="f16s3", **attrs):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / "net.cfg"), cfg_text), True)          # no .eval(): the statistics of the batch
    assert m.training
    m.net_info["height"] = res
    m.precision = precision
    m.options = dict(options, bn_batch_split=1)
    m.keep_all_layers = True
    m.autotune = False
    m.update_running_stats = False
    for k, v in attrs.items():
        setattr(m, k, v)
    m.load_weight_stream(wts)
    return m


def _forward(m, xg):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                      # the training-mode warning (checked end to end below)
        return m(xg).clone()


def _stored(m, B):
    torch.cuda.synchronize()
    out = {}
    for D in m.plan_description()["layers"]:
        if D["type"] == "yolo" or (D["type"] == "convolutional" and D["fused_into"] >= 0):
            continue                                                          # (a single-source route reads back the layer it aliases)
        out[D["index"]] = m.read_layer(D["index"], B).cpu()
    return out


def _stats(m, ref):
    """(mean, var) float64 arrays of every BatchNorm conv of the last forward."""
    lib = _ffi.lib()
    out = {}
    for c, _, _, _ in bn_layers(ref):
        n = ref.ir.layers[c].cout
        mean, var = np.empty(n, np.float64), np.empty(n, np.float64)
        _ffi.check(lib.rtod_plan_bn_batch_stats(m._plan, c, mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), n, None))
        out[c] = (mean, var)
    return out


def _same(tag, a, b):
    ya, la, sa = a
    yb, lb, sb = b
    assert torch.equal(ya, yb), (tag, "output")
    assert la.keys() == lb.keys()
    for i in la:
        assert torch.equal(la[i], lb[i]), (tag, "layer", i)
    for c in sa:
        assert np.array_equal(sa[c][0], sb[c][0]) and np.array_equal(sa[c][1], sb[c][1]), (tag, "statistics of layer", c)


def _gate_bn_layers(tag, ref, x, stored, stats, ids=None):
    """The model of every BatchNorm conv from the GPU's stored inputs; -> number of layers gated."""
    failed = []
    n = 0
    for c, s, src, r in bn_layers(ref):
        L = ref.ir.layers[c]
        a = x if src < 0 else stored[src]
        res = None if r is None else stored[r]
        with torch.no_grad():
            rec = bn_layer_model(L, ref.params[c], a, res, references=True)
        got = stored[s]
        assert torch.isfinite(got).all(), (tag, s)
        rr = residual(got, rec)
        fl = floors(rec)
        ok, q_rms, q_max = gate(rr, fl)
        mean, var = stats[c]
        dm = float(np.abs(mean - rec["mean"].numpy()).max() / max(1e-30, float(rec["var"].sqrt().max())))
        print("GATE %s layer %d conv %dx%d/%d Cin %d Cout %d map %dx%d %s: rms/D %.3e (%.2f F_rms) max/D %.3e (%.2f F_max), mean off by %.1e sigma%s"
              % (tag, s, L.size, L.size, L.stride, L.cin, L.cout, L.hout, L.wout, "" if ids is None or c not in ids else "ids %s" % (ids[c],),
                 rms_max(rr)[0], q_rms, rms_max(rr)[1], q_max, dm, "" if ok else "  EXCEEDS THE GATE at %s" % (np.unravel_index(np.abs(rr).argmax(), rr.shape),)))
        if not ok:
            failed.append((s, q_rms, q_max))
        n += 1
    assert not failed, "%s: layers outside the gate (layer, rms / F_rms, max / F_max): %s" % (tag, failed)
    return n


_runs = {}


def _probe_run(name, d):
    """One prepared plan of the probe: the default tile table's forward, then every accepted id of the conv under test."""
    if name in _runs:
        return _runs[name]
    p = BY_NAME[name]
    ref, wts, x = setup(p)
    xg = x.cuda()
    m = _model(p.cfg(), p.H, d, wts, p.options)
    m.prepare(p.B, xg.device)
    assert m.active_precision == "f16s3"
    n = m._info.n_launches
    launch = launch_of_layer(m.launch_infos(), p.conv_layer)
    ids = accepted_ids(_ffi.lib(), m._plan, n, launch, p.B)
    assert ids and ids == legal_ids(p, 2), (name, ids)                        # the plain-f16 set of the same probe (host test)
    want = (_forward(m, xg), _stored(m, p.B), _stats(m, ref))
    default = m.launch_infos()[launch].variant - 100
    assert default in ids
    _runs[name] = (p, ref, x, xg, m, launch, ids, want)
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_probe_layer_local_model(tmp_path_factory, name):
    p, ref, x, xg, m, launch, ids, want = _probe_run(name, tmp_path_factory.mktemp("bn"))
    y, stored, stats = want
    assert p.stored_layer in stored and not m.overflowed()
    assert _gate_bn_layers("probe " + name, ref, x, stored, stats) == p.conv_layer + 1
    # the head (no BatchNorm, fused decode) runs as in an eval plan: the output against the oracle in the same mode
    with torch.no_grad():
        ref_y = ref.forward(x, batch_stats=True)
    e = rel_err(y.cpu().numpy(), ref_y.numpy())
    print("PROBE %s: output max rel err %.2e vs the float32 oracle on batch statistics" % (name, float(e.max())))


@pytest.mark.parametrize("name", NAMES)
def test_probe_every_legal_tile_gives_the_layers_bits(tmp_path_factory, name):
    p, ref, x, xg, m, launch, ids, want = _probe_run(name, tmp_path_factory.mktemp("bn"))
    n = m._info.n_launches
    fams = sorted(f for f, r in FAMILIES.items() if set(ids) & set(r))
    print("PROBE %s (%s): families %s, ids %s" % (name, p.note, fams, ids))
    for v in ids:
        table = [-1] * n
        table[launch] = v
        m.set_tiles(p.B, table)
        got = (_forward(m, xg), _stored(m, p.B), _stats(m, ref))
        assert m.launch_infos()[launch].variant == 100 + v, (name, v)          # the id really ran
        _same((name, "tile", v), got, want)
        again = (_forward(m, xg), _stored(m, p.B), _stats(m, ref))
        _same((name, "tile", v, "second forward"), again, want)
    assert not m.overflowed()
    m.set_tiles(p.B, [-1] * n)
    run = m.make_graphed(xg)
    yg, _ = run(xg)
    torch.cuda.synchronize()
    _same((name, "graph replay"), (yg.clone(), _stored(m, p.B), _stats(m, ref)), want)


@pytest.mark.parametrize("B", [2, 3])
def test_mini_cfg_layer_local_model(tmp_path_factory, B):
    """2x2 grid at the deepest stage (8 or 12 samples per channel), a stride-2 producer writing into a zero-copy concat at
    coff > 0, a shortcut and two heads."""
    text = cfgs.mini_cfg(64, 64)
    ref = O.RefDarknet(text, 64)
    wts = synth.synth_weights(ref.ir)
    ref.load_weight_stream(wts)
    x = torch.from_numpy(synth.synth_frames(B, 64, seed=9))
    m = _model(text, 64, tmp_path_factory.mktemp("mini"), wts)
    y = _forward(m, x.cuda())
    assert m.active_precision == "f16s3" and torch.isfinite(y).all() and not m.overflowed()
    desc = m.plan_description()
    assert any(D["coff"] > 0 and D["type"] == "convolutional" and D["stride"] == 2 for D in desc["layers"])
    tiles = {li.layer: li.variant - 100 for li in m.launch_infos() if li.kind == 0 and li.variant >= 100}
    n = _gate_bn_layers("mini_cfg B%d" % B, ref, x, _stored(m, B), _stats(m, ref), tiles)
    assert n == len(bn_layers(ref)) == 15


@pytest.mark.parametrize("res,B", [(416, 2), (320, 3)])
def test_end_to_end_vs_reference_golden(golden_dir, tmp_path_factory, res, B):
    from realtimeobjectdetection_amd.darknet import Darknet
    g = np.load(os.path.join(golden_dir, "trainbn.npz"))
    tag = "yolov3_%d_b%d" % (res, B)
    cfg_text = NETS["yolov3"]()
    d = tmp_path_factory.mktemp("e2e_" + tag)
    ref = O.RefDarknet(cfg_text, res)
    w = synth.synth_weights(ref.ir)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=31))
    stride = int(g["stride_" + tag])
    fig = {}
    for path in ("fp32", "split"):
        m = Darknet(cfgs.write_cfg(str(d / ("yolov3_%s.cfg" % path)), cfg_text), True)   # no .eval(), precision "auto": as detect.py builds it
        assert m.training and m.precision == "auto"
        m.net_info["height"] = res
        if path == "split":
            m.options = {"bn_batch_split": 1}
        m.load_weight_stream(w)
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="training mode"):
            y = m(x.cuda())
        assert m.active_precision == ("f16s3" if path == "split" else "fp32")
        e = rel_err(y.cpu().numpy()[:, ::stride], g["rows_" + tag])
        fig[path] = (float(np.quantile(e, 0.999)), float(e.max()))
        if path == "fp32":
            del m
    print("E2E %s: split p99.9 %.2e max %.2e | fp32 batch-BN p99.9 %.2e max %.2e (gate 1e-4 / 3.5e-4)" % ((tag,) + fig["split"] + fig["fp32"]))
    assert fig["split"][0] <= TOL and fig["split"][1] <= 3.5e-4, "p99.9 %.3e max %.3e" % fig["split"]
    assert not m.overflowed()
    bns = [(i, mod) for i, seq in enumerate(m.module_list) for mod in seq.children() if isinstance(mod, torch.nn.BatchNorm2d)]
    for i, bn in (bns[0], bns[-1]):
        assert np.allclose(bn.running_mean.cpu().numpy(), g["rmean_%s_L%d" % (tag, i)], rtol=1e-4, atol=1e-6)
        assert np.allclose(bn.running_var.cpu().numpy(), g["rvar_%s_L%d" % (tag, i)], rtol=1e-4, atol=1e-6)
        assert int(bn.num_batches_tracked) == 1
    m.update_running_stats = False
    with torch.no_grad():
        y1 = m(x[:1].cuda())
    assert not torch.equal(y1[0], y[0])                                      # the result depends on the batch
    m.eval()                                                                 # ... and eval() afterwards is the folded path
    with torch.no_grad():
        ye = m(x.cuda())
    assert m.active_precision == "f16s3" and "bn_raw_bytes" not in m.plan_description()
    assert torch.isfinite(ye).all() and not torch.equal(ye, y) and not m.overflowed()


def test_tiny_falls_back_to_fp32(golden_dir, tmp_path_factory):
    from realtimeobjectdetection_amd.darknet import Darknet
    g = np.load(os.path.join(golden_dir, "trainbn.npz"))
    tag = "yolov3-tiny_416_b2"
    cfg_text = NETS["yolov3-tiny"]()
    d = tmp_path_factory.mktemp("e2e_tiny")
    for options in ({"bn_batch_split": 1}, {"bn_batch_split": 1, "narrow_cin": 1}):
        m = Darknet(cfgs.write_cfg(str(d / "tiny.cfg"), cfg_text), True)
        m.net_info["height"] = 416
        m.options = dict(options)
        ref = O.RefDarknet(cfg_text, 416)
        m.load_weight_stream(synth.synth_weights(ref.ir))
        x = torch.from_numpy(synth.synth_frames(2, 416, seed=31))
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="training mode"):
            y = m(x.cuda())
        assert m.active_precision == "fp32"
        e = rel_err(y.cpu().numpy()[:, ::int(g["stride_" + tag])], g["rows_" + tag])
        assert np.quantile(e, 0.999) <= TOL and e.max() <= 3.5e-4, "p99.9 %.3e max %.3e" % (float(np.quantile(e, 0.999)), float(e.max()))
    m.precision = "f16"
    with pytest.raises(RuntimeError):
        m(x.cuda())
