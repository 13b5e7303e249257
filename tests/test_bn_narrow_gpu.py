"""GPU tests of batch-statistics BatchNorm on the narrow split-f16 kernels (Darknet.options = {"narrow_cin": 1, "stem_pool": 1,
"bn_batch_split": 1, "bn_split_narrow": 1}, module in training mode, precision "f16s3" / "auto"): YOLOv3-tiny's kind of graph.
Run on an MI355X with ``pytest -m gpu``.

1. Layer-local float64 model (tests/bn_narrow_model.py) on every narrow probe, on narrow_mini_cfg at 64x64 (B = 2, 3) and on
   bn_pool_mini_cfg at 64x64 B = 1 and 40x40 B = 3, keep_all_layers on: every stored BatchNorm layer is recomputed from the GPU's
   OWN stored input and shortcut operand and held to f16s3_emulation.gate (GATE_M = 4 times the floors of three float32 evaluations
   of the same layer); layer 0 runs the 16-filter split stem and is held to the split-stem model; the batch means lie within
   bn_narrow_model.mean_tolerance of the model's (a bound from the format alone).
2. Every tile id rtod_plan_set_tiles accepts for a probe's conv under test — the narrow family, nothing else — gives the default
   tile's bits: stored layers, output and the batch statistics of every BatchNorm layer; a second forward and a HIP-graph replay
   repeat them.
3. bn_pool_mini_cfg and stem_pool_mini_cfg (with the split stem, and with layer 0 on the exact-fp32 kernel), 64x64 B = 1 and 40x40
   B = 3: the plan that normalises and pools in one kernel against fuse_bn_pool = 0 and against keep_all_layers — output, every
   layer both plans hold after the forward, all batch statistics and the range flag bitwise equal; again with one channel's beta
   at +1e4 and one at -1e5 on a fused layer (positive and negative saturation): the flag raised in every plan, the output finite.
4. End to end, the whole as-run path: YOLOv3-tiny 416 B = 2, no .eval(), precision "auto", against tests/golden/trainbn.npz;
   the exact-fp32 as-run plan is measured in the same test.  The gate is the mode's documented one (p99.9 <= 1e-4, max <= 3.5e-4:
   test_gpu_parity.py).
   MEASURED (MI355X; rel_err against the golden rows, p99.9 / max):
       yolov3-tiny_416_b2   split 1.62e-05 / 3.26e-05    fp32 batch-BN 1.35e-05 / 3.68e-05
   Layer by layer the kernels sit at 0.4-0.8x the float32 floors in rms and at most 1.5x in max (gate: 4x); the batch means at
   most 0.03 of their bound.

Every test prints its figures ("GATE ..." / "E2E ..." lines).
"""
import os

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from oracle import darknet_ref as O
from bn_narrow_model import BY_NAME, NARROW, NARROW_OPTIONS, bn_layers, mean_tolerance, narrow_layer_model, stem_is_split
from conv_probes import FAMILIES, accepted_ids, launch_of_layer, setup
from f16s3_emulation import floors, gate, residual, rms_max
from test_bn_split_gpu import _forward, _model, _same, _stats, _stored
from test_gpu_parity import rel_err
from test_oracle_golden import NETS

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = [p.name for p in NARROW]
OPTS = dict(NARROW_OPTIONS)
NO_STEM16 = {k: v for k, v in OPTS.items() if k != "stem_pool"}
SHAPES = [(64, 1), (40, 3)]


def _gate_bn_layers(tag, ref, x, stored, stats, options):
    """The model of every BatchNorm conv from the GPU's stored inputs; -> number of layers gated."""
    failed = []
    n = 0
    split0 = stem_is_split(ref.ir, options)
    for c, s, src, r in bn_layers(ref):
        L = ref.ir.layers[c]
        a = x if src < 0 else stored[src]
        res = None if r is None else stored[r]
        with torch.no_grad():
            rec = narrow_layer_model(L, ref.params[c], a, res, references=True, split_stem=split0)
        got = stored[s]
        assert torch.isfinite(got).all(), (tag, s)
        rr = residual(got, rec)
        ok, q_rms, q_max = gate(rr, floors(rec))
        mean, var = stats[c]
        dm = np.abs(mean - rec["mean"].numpy()) / mean_tolerance(rec).numpy()
        mean_ok = bool((dm <= 1.0).all())
        print("GATE %s layer %d conv %dx%d/%d Cin %d Cout %d map %dx%d%s: rms/D %.3e (%.2f F_rms) max/D %.3e (%.2f F_max), mean off by %.3f of its bound%s"
              % (tag, s, L.size, L.size, L.stride, L.cin, L.cout, L.hout, L.wout, " (split stem)" if c == 0 and split0 else "",
                 rms_max(rr)[0], q_rms, rms_max(rr)[1], q_max, float(dm.max()), "" if ok and mean_ok else "  EXCEEDS THE GATE"))
        if not (ok and mean_ok):
            failed.append((s, q_rms, q_max, float(dm.max())))
        n += 1
    assert not failed, "%s: layers outside the gate (layer, rms / F_rms, max / F_max, mean / bound): %s" % (tag, failed)
    return n


_runs = {}


def _probe_run(name, d):
    """One prepared plan of the probe: the default tile table's forward."""
    if name in _runs:
        return _runs[name]
    p = BY_NAME[name]
    ref, wts, x = setup(p)
    xg = x.cuda()
    m = _model(p.cfg(), p.H, d, wts, p.options)
    m.prepare(p.B, xg.device)
    assert m.active_precision == "f16s3"
    infos = m.launch_infos()
    assert infos[0].kind == 7                                                  # the 16-filter split stem, no pack launch
    launch = launch_of_layer(infos, p.conv_layer)
    ids = accepted_ids(_ffi.lib(), m._plan, m._info.n_launches, launch, p.B)
    assert ids == list(FAMILIES["narrow"]), (name, ids)
    want = (_forward(m, xg), _stored(m, p.B), _stats(m, ref))
    assert m.launch_infos()[launch].variant - 100 in ids
    _runs[name] = (p, ref, x, xg, m, launch, ids, want)
    return _runs[name]


# ------------------------------------------------------------------------------- 1. the layer-local model
@pytest.mark.parametrize("name", NAMES)
def test_probe_layer_local_model(tmp_path_factory, name):
    p, ref, x, xg, m, launch, ids, want = _probe_run(name, tmp_path_factory.mktemp("bnn"))
    y, stored, stats = want
    assert p.stored_layer in stored and not m.overflowed()
    assert _gate_bn_layers("probe " + name, ref, x, stored, stats, p.options) == len(bn_layers(ref))
    with torch.no_grad():
        ref_y = ref.forward(x, batch_stats=True)
    e = rel_err(y.cpu().numpy(), ref_y.numpy())
    print("PROBE %s: output max rel err %.2e vs the float32 oracle on batch statistics" % (name, float(e.max())))


_nets = {}


def _net(kind, res):
    """(cfg text, oracle with the synthetic weights, weight stream) of a test graph: built once, never modified."""
    if (kind, res) not in _nets:
        text = {"narrow_mini": cfgs.narrow_mini_cfg, "bn_pool_mini": cfgs.bn_pool_mini_cfg, "stem_pool_mini": cfgs.stem_pool_mini_cfg}[kind](res, res)
        ref = O.RefDarknet(text, res)
        wts = synth.synth_weights(ref.ir)
        ref.load_weight_stream(wts)
        _nets[(kind, res)] = (text, ref, wts)
    return _nets[(kind, res)]


@pytest.mark.parametrize("kind,res,B", [("narrow_mini", 64, 2), ("narrow_mini", 64, 3), ("bn_pool_mini", 64, 1), ("bn_pool_mini", 40, 3)])
def test_mini_cfgs_layer_local_model(tmp_path_factory, kind, res, B):
    text, ref, wts = _net(kind, res)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=9))
    m = _model(text, res, tmp_path_factory.mktemp("mini"), wts, OPTS)
    y = _forward(m, x.cuda())
    assert m.active_precision == "f16s3" and torch.isfinite(y).all() and not m.overflowed()
    desc = m.plan_description()
    assert all(D["fused_into"] < 0 or desc["layers"][D["fused_into"]]["type"] != "maxpool" for D in desc["layers"])     # keep_all_layers: stand-alone pools
    assert m.launch_infos()[0].kind == 7
    n = _gate_bn_layers("%s %d B%d" % (kind, res, B), ref, x, _stored(m, B), _stats(m, ref), OPTS)
    assert n == len(bn_layers(ref))


# ------------------------------------------------------------------------------- 2. every tile, a second forward, a graph replay
@pytest.mark.parametrize("name", NAMES)
def test_probe_every_legal_tile_gives_the_layers_bits(tmp_path_factory, name):
    p, ref, x, xg, m, launch, ids, want = _probe_run(name, tmp_path_factory.mktemp("bnn"))
    n = m._info.n_launches
    print("PROBE %s (%s): ids %s" % (name, p.note, ids))
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


# ------------------------------------------------------------------------------- 3. normalise + pool in one kernel == stand-alone
def _intact(m, layer, B):
    """True when no buffer written after ``layer``'s last reader shares its arena range (read_layer is then valid without keep_all_layers)."""
    d = m.plan_description()
    bufs = d["bufs"]
    bi = d["layers"][layer]["buf"]
    if bi < 0:
        return False
    b = bufs[bi]
    lo, hi = b["offset"], b["offset"] + b["floats_per_frame"] * B
    for i, o in enumerate(bufs):
        if i == bi or o["last"] <= b["last"]:
            continue
        if o["offset"] < hi and lo < o["offset"] + o["floats_per_frame"] * B:
            return False
    return True


def _with_beta(ref, wts, layer, values):
    """Copy of the stream with beta of ``layer`` replaced at the given channels."""
    start = synth.conv_weight_slices(ref.ir)[layer][0] - 4 * ref.ir.layers[layer].cout      # beta, gamma, mean, var, weights
    out = wts.copy()
    for ch, v in values.items():
        out[start + ch] = np.float32(v)
    return out


@pytest.mark.parametrize("saturate", [False, True])
@pytest.mark.parametrize("res,B", SHAPES)
@pytest.mark.parametrize("kind,options,fused_convs", [("bn_pool_mini", OPTS, (0, 2, 4)), ("stem_pool_mini", OPTS, (0,)), ("stem_pool_mini", NO_STEM16, (0,))])
def test_fused_pool_equals_stand_alone_bitwise(tmp_path_factory, kind, options, fused_convs, res, B, saturate):
    text, ref, wts = _net(kind, res)
    sat_layer = fused_convs[min(1, len(fused_convs) - 1)]                      # bn_pool_mini: the Cin-16 conv; stem_pool_mini: layer 0
    if saturate:
        wts = _with_beta(ref, wts, sat_layer, {3: 1e4, 5: -1e5})
    x = torch.from_numpy(synth.synth_frames(B, res, seed=9)).cuda()
    d = tmp_path_factory.mktemp("fp")
    kw = dict(overflow_check="off")
    fused = _model(text, res, d, wts, options, keep_all_layers=False, **kw)
    plain = _model(text, res, d, wts, dict(options, fuse_bn_pool=0), keep_all_layers=False, **kw)
    keep = _model(text, res, d, wts, dict(options, fuse_bn_pool=0), **kw)
    ys = [_forward(m, x) for m in (fused, plain, keep)]
    torch.cuda.synchronize()
    flags = [m.overflowed() for m in (fused, plain, keep)]
    assert all(m.active_precision == "f16s3" for m in (fused, plain, keep))
    assert (fused.launch_infos()[0].kind == 7) == ("stem_pool" in options)     # the split stem, or (pack +) the exact-fp32 conv
    form = lambda m: tuple(D["index"] for D in m.plan_description()["layers"] if D["type"] == "convolutional" and D["bn"] and D["fused_into"] >= 0)
    assert form(fused) == fused_convs and form(plain) == () and form(keep) == ()
    assert torch.isfinite(ys[0]).all()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert flags == [saturate] * 3, flags
    sf, sp, sk = _stats(fused, ref), _stats(plain, ref), _stats(keep, ref)
    for c in sk:
        for s in (sf, sp):
            assert np.array_equal(s[c][0], sk[c][0]) and np.array_equal(s[c][1], sk[c][1]), (kind, "statistics of layer", c)
    compared = []
    for D in fused.plan_description()["layers"]:
        i = D["index"]
        if D["type"] == "yolo" or (D["type"] == "convolutional" and D["fused_into"] >= 0) or not _intact(fused, i, B):
            continue
        got, want = fused.read_layer(i, B), keep.read_layer(i, B)
        assert got.shape == want.shape and torch.equal(got, want), (kind, "layer", i, int((got != want).sum()))
        compared.append(i)
    print("FUSED %s %d B%d%s: fused convs %s, layers compared bitwise %s" % (kind, res, B, " saturated" if saturate else "", fused_convs, compared))
    assert any(i - 1 in fused_convs for i in compared), compared                # at least one pooled map itself
    with pytest.raises(RuntimeError):
        fused.read_layer(fused_convs[0], B)                                    # never stored


# ------------------------------------------------------------------------------- 4. end to end
def test_tiny_end_to_end_vs_reference_golden(golden_dir, tmp_path_factory):
    """YOLOv3-tiny as its callers run it.  Fails without the feature (the option name is unknown to rtod_plan_set_option)."""
    from realtimeobjectdetection_amd.darknet import Darknet
    g = np.load(os.path.join(golden_dir, "trainbn.npz"))
    res, B = 416, 2
    tag = "yolov3-tiny_%d_b%d" % (res, B)
    cfg_text = NETS["yolov3-tiny"]()
    d = tmp_path_factory.mktemp("e2e_" + tag)
    ref = O.RefDarknet(cfg_text, res)
    w = synth.synth_weights(ref.ir)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=31))
    stride = int(g["stride_" + tag])
    fig = {}
    for path in ("fp32", "split"):
        m = Darknet(cfgs.write_cfg(str(d / ("tiny_%s.cfg" % path)), cfg_text), True)     # no .eval(), precision "auto": as detect.py builds it
        assert m.training and m.precision == "auto"
        m.net_info["height"] = res
        if path == "split":
            m.options = {"narrow_cin": 1, "stem_pool": 1, "bn_batch_split": 1, "bn_split_narrow": 1}    # (bn_batch_stats: set by the training mode)
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
    desc = m.plan_description()
    assert [desc["layers"][i]["fused_into"] for i in (0, 2, 4, 6, 8, 10)] == [1, 3, 5, 7, -1, -1]
    bns = [(i, mod) for i, seq in enumerate(m.module_list) for mod in seq.children() if isinstance(mod, torch.nn.BatchNorm2d)]
    assert (bns[0][0], bns[-1][0]) == (0, 21)
    for i, bn in (bns[0], bns[-1]):
        assert np.allclose(bn.running_mean.cpu().numpy(), g["rmean_%s_L%d" % (tag, i)], rtol=1e-4, atol=1e-6)
        assert np.allclose(bn.running_var.cpu().numpy(), g["rvar_%s_L%d" % (tag, i)], rtol=1e-4, atol=1e-6)
        assert int(bn.num_batches_tracked) == 1
    m.update_running_stats = False
    with torch.no_grad():
        y1 = m(x[:1].cuda())
    assert not torch.equal(y1[0], y[0])                                        # the result depends on the batch
    m.eval()                                                                   # ... and eval() afterwards is the folded plan
    with torch.no_grad():
        ye = m(x.cuda())
    assert m.active_precision == "f16s3" and "bn_raw_bytes" not in m.plan_description()
    assert torch.isfinite(ye).all() and not torch.equal(ye, y) and not m.overflowed()
