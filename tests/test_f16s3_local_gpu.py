"""GPU tests that hold every split-f16 conv tile to the float64 model of the format, layer by layer.  Run on an MI355X with
``pytest -m gpu``.

The cumulative gates (2e-5 of a layer's abs-max against the float32 oracle, 1e-4 on the output) carry the error of a whole
network normalised by its largest element, and bit identity between tiles only proves that tiles agree.  Here every stored
conv layer is recomputed by tests/f16s3_emulation.py from the GPU's OWN stored inputs (``feed``), so the distance is that
layer's arithmetic alone, and is measured per element in units of D = conv(|a|, |w|) + |bias| + |shortcut operand|:
r = (value - model) / D.  The gate (f16s3_emulation.gate, shared with the CPU teeth test) is

    rms(r_gpu) <= 4 F_rms   and   max |r_gpu| <= 4 F_max

where F_rms / F_max are the largest rms / max of r over three float32 evaluations of the same layer from the same inputs
(torch NCHW, torch channels_last, 32-channel K chunks in the kernels' order).  tests/test_f16s3_emulation_host.py proves on the
CPU that every listed mutant of the model fails this gate on every probe.

* Per probe (tests/conv_probes.py), f16s3: every tile id rtod_plan_set_tiles accepts for the conv under test runs through a
  tile table on one prepared plan; launch_infos() must report that id; every stored layer and the output must have the same
  bits for every id; frame i alone must give row i of the batch; the emulation is evaluated once per probe and gated on every
  stored conv layer; the decoded output passes the existing 1e-4 gate against the float32 oracle; no overflow.
* Per probe, f16: the same enumeration (smaller legal sets), bit identity, and the existing layer-local gate of
  tests/test_narrow_gpu.py (_check_layer_local) unchanged.
* Whole graphs, f16s3, autotuned tiles: YOLOv3 at 160x160 batch 2, the YOLOv5s-shaped graph at 128x128 batch 3 and mini_cfg at
  96x96 batch 2, the gate on every stored conv layer; routes, max-pools and nearest upsampling bit for bit; bilinear upsampling
  within its one store rounding.

keep_all_layers (needed to read the layers back) switches off the fused stem + layer 1 kernel and the stem's max-pool
fusion: those stay covered by their bit-identity tests against the unfused kernels (tests/test_gpu_parity.py,
tests/test_stem_pool_gpu.py), which this module does not replace.  The hosted 1x1 epilogue stays on (Plan::pw_active does not
look at keep_all_layers): a hosted 1x1 conv stores its output like any other, so the whole graphs gate it ("hosted" in the
printed lines), and the one probe whose conv under test would be hosted (slab_c64) switches option fuse_pointwise off so that
the launch under test runs.  Heads with a fused decode are not materialised in split plans: their arithmetic is covered by
the output gate.

Every test prints its per-layer figures ("GATE ..." lines; profiles/experiments/f16s3_layer_local.log is one run's output).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from realtimeobjectdetection_amd import cfgs, synth
from oracle import darknet_ref as O
from conv_probes import PROBES, BY_NAME, FAMILIES, accepted_ids, launch_of_layer, legal_ids, setup
from f16_emulation import rel
from f16s3_emulation import F16S3Emulation, floors, gate, residual, rms_max
from rect_ref import forward_rect, predict_transform_rect
from test_narrow_gpu import _check_layer_local, _materialised

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = [p.name for p in PROBES]


def _model(cfg_text, h, w, precision, d, wts, options=(), **attrs):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / "net.cfg"), cfg_text), True).eval()
    m.net_info["height"] = h
    if w != h:
        m.input_width = w
    m.precision = precision
    m.options = dict(options)
    m.keep_all_layers = True
    for k, v in attrs.items():
        setattr(m, k, v)
    m.load_weight_stream(wts)
    return m


def _stored(m, B):
    """Every materialised layer of the last forward that owns its buffer: index -> tensor on the host."""
    torch.cuda.synchronize()
    return {D["index"]: m.read_layer(D["index"], B).cpu() for D in _materialised(m) if D["alias_of"] < 0}


def _families(ids):
    return sorted(f for f, r in FAMILIES.items() if set(ids) & set(r))


def _gate_every_layer(tag, ref, options, x, stored, ids):
    """The emulation, once, from the GPU's stored inputs; the gate on every stored conv layer; data movement bit for bit.
    ``ids``: conv layer -> what ran there, for the printed line.  -> number of conv layers gated"""
    emu = F16S3Emulation(ref, options)
    for i, t in stored.items():
        assert torch.isfinite(t).all(), (tag, i)
    with torch.no_grad():
        _, model, recs = emu.forward(x, feed=stored, keep_layers=True, records=True, references=True)
    failed = []
    for i, got in sorted(stored.items()):
        L = ref.ir.layers[i]
        if i in recs:
            rec = recs[i]
            c = ref.ir.layers[rec["conv"]]
            r = residual(got, rec)
            fl = floors(rec)
            ok, q_rms, q_max = gate(r, fl)
            print("GATE %s layer %d conv %dx%d/%d Cin %d Cout %d map %dx%d ids %s: rms/D %.3e (%.2f F_rms) max/D %.3e (%.2f F_max)%s"
                  % ((tag, i, c.size, c.size, c.stride, c.cin, c.cout, c.hout, c.wout, ids.get(rec["conv"], "default")) + (rms_max(r)[0], q_rms, rms_max(r)[1], q_max)
                     + ("" if ok else "  EXCEEDS THE GATE at %s" % (np.unravel_index(np.abs(r).argmax(), r.shape),),)))
            if not ok:
                failed.append((i, q_rms, q_max))
            continue
        assert L.type != "convolutional", (tag, i, "a stored conv layer the model did not evaluate")
        want = model[i]
        if L.type == "upsample" and not L.nearest:
            # one float32 evaluation (weights 9/16, 3/16, 3/16, 1/16: exact products, three roundings of 2^-24) and one store
            # split (22 bits) against the model's: 2^-20 of the interpolated magnitudes, plus one quantum of a subnormal lo
            # half (2^-24 / 8)
            bound = 2.0 ** -20 * F.interpolate(stored[i - 1].double().abs(), scale_factor=2, mode="bilinear", align_corners=False) + 2.0 ** -26
            assert bool(((got.double() - want).abs() <= bound).all()), (tag, i, "bilinear upsample")
        else:
            assert torch.equal(got.double(), want), (tag, i, L.type)           # route, max-pool, nearest upsampling: the same bits
    assert not failed, "%s: layers outside the gate (layer, rms / F_rms, max / F_max): %s" % (tag, failed)
    return len(recs)


def _run_every_id(p, precision, d):
    """One prepared plan of the probe, every legal id of the conv under test through a tile table.
    -> (model, ids, output of the batch, stored layers)"""
    ref, wts, x = setup(p)
    xg = x.cuda()
    m = _model(p.cfg(), p.H, p.W, precision, d, wts, p.options, autotune=False)
    m.prepare(p.B, xg.device)
    n = m._info.n_launches
    launch = launch_of_layer(m.launch_infos(), p.conv_layer)
    from realtimeobjectdetection_amd import _ffi
    ids = accepted_ids(_ffi.lib(), m._plan, n, launch, p.B)
    assert ids and ids == legal_ids(p, 1 if precision == "f16s3" else 2), (p.name, ids)
    want_y = want = None
    for v in ids:
        table = [-1] * n
        table[launch] = v
        m.set_tiles(p.B, table)
        with torch.no_grad():
            y = m(xg).clone()
        assert m.launch_infos()[launch].variant == 100 + v, (p.name, v, m.launch_infos()[launch].variant)   # the id really ran
        layers = _stored(m, p.B)
        assert not m.overflowed(), (p.name, v)
        if want is None:
            want_y, want = y, layers
            assert p.stored_layer in want and p.conv_layer - 1 in want
            continue
        assert torch.equal(y, want_y), (p.name, v)
        for i, t in layers.items():
            assert torch.equal(t, want[i]), (p.name, "tile", v, "layer", i)
    # frame i alone == row i of the batch (the tile table of batch 1 is the closed-form default)
    for i in range(p.B):
        with torch.no_grad():
            yi = m(xg[i:i + 1]).clone()
        assert torch.equal(yi[0], want_y[i]), (p.name, "frame", i)
        one = _stored(m, 1)
        for k, t in one.items():
            assert torch.equal(t[0], want[k][i]), (p.name, "frame", i, "layer", k)
    assert m.active_precision == precision and not m.overflowed()
    return m, ids, want_y, want


@pytest.mark.parametrize("name", NAMES)
def test_probe_f16s3_every_tile_same_bits_and_inside_the_gate(tmp_path_factory, name):
    p = BY_NAME[name]
    ref, wts, x = setup(p)
    m, ids, y, stored = _run_every_id(p, "f16s3", tmp_path_factory.mktemp("pl"))
    print("PROBE %s (%s): conv under test layer %d, families %s, ids %s" % (p.name, p.note, p.conv_layer, _families(ids), ids))
    n = _gate_every_layer("probe " + p.name, ref, p.options, x, stored, {p.conv_layer: "every id of " + "+".join(_families(ids))})
    assert n == p.conv_layer + 1                              # the stem, the optional 1x1 and the conv under test
    with torch.no_grad():
        want = forward_rect(ref, x)
    e = rel(y.cpu().numpy(), want.numpy())
    assert y.shape == want.shape and e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


@pytest.mark.parametrize("name", NAMES)
def test_probe_f16_every_tile_same_bits_and_layer_local_gate(tmp_path_factory, monkeypatch, name):
    # the f16 emulation decodes heads with the oracle's square predict_transform; rect_ref's is the same arithmetic on a GH x GW grid
    monkeypatch.setattr(O, "predict_transform", predict_transform_rect)
    p = BY_NAME[name]
    ref, wts, x = setup(p)
    m, ids, y, stored = _run_every_id(p, "f16", tmp_path_factory.mktemp("pf"))
    print("PROBE f16 %s: families %s, ids %s" % (p.name, _families(ids), ids))
    table = [-1] * m._info.n_launches
    m.set_tiles(p.B, table)
    with torch.no_grad():
        y = m(x.cuda())
    torch.cuda.synchronize()
    _check_layer_local(m, ref, x, y, p.B, p.conv_layer + 1)


GRAPHS = {
    "yolov3_160_b2": (lambda: cfgs.yolov3_cfg(160, 160), 160, 2, 72),          # 75 convs - 3 fused head convs; 23 of them stored through their shortcut
    "yolov5s_128_b3": (lambda: cfgs.yolov5s_style_cfg(128, 128), 128, 3, 57),
    "mini_96_b2": (lambda: cfgs.mini_cfg(96, 96), 96, 2, 15),
}


@pytest.mark.parametrize("tag", sorted(GRAPHS))
def test_whole_graph_f16s3_autotuned_tiles_inside_the_gate_layer_by_layer(tmp_path_factory, tag):
    text, res, B, n_convs = GRAPHS[tag]
    ref = O.RefDarknet(text(), res)
    wts = synth.synth_weights(ref.ir)
    ref.load_weight_stream(wts)
    x = torch.from_numpy(synth.synth_frames(B, res, seed=9))
    m = _model(text(), res, res, "f16s3", tmp_path_factory.mktemp("wg"), wts)
    with torch.no_grad():
        y = m(x.cuda())                                      # autotunes this batch size
        want = ref.forward(x)
    stored = _stored(m, B)
    assert m.active_precision == "f16s3" and not m.overflowed()
    tile_of = {li.layer: li.variant - 100 if li.variant >= 100 else "hosted" if li.variant < 0 else "stem / exact-fp32" for li in m.launch_infos() if li.kind in (0, 7)}
    print("GRAPH %s: tiles in use %s" % (tag, sorted({v for v in tile_of.values() if isinstance(v, int)})))
    assert _gate_every_layer("graph " + tag, ref, (), x, stored, tile_of) == n_convs
    e = rel(y.cpu().numpy(), want.numpy())
    assert e.max() <= TOL, f"max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"
