"""GPU tests that hold every instantiation of the exact-fp32 conv kernel (csrc/conv_igemm_f32.hip: tiles 128x128, 128x64,
64x64, 128x32 x MODE 0 one chain / MODE 1 slices inside the workgroup / MODE 2 a workgroup per slice + conv_slice_reduce_kernel)
to float64 probes.  Run on an MI355X with ``pytest -m gpu``.

Per probe (tests/f32_probes.py) one model per tile (option force_f32_variant 0..3) x schedule ({"k_slices": 0},
{"k_slice_workgroups": 0}, default), keep_all_layers, autotune off: twelve small plans.

a. The instantiation ran: launch_infos() reports tile + 10 * mode for the conv under test (mode 0 under k_slices = 0 or where
   the planner's rule does not slice the layer, 1 under k_slice_workgroups = 0, 2 by default); over all probes the twelve ids
   all occur (test_the_probes_run_all_twelve_instantiations).
b. Same bits: every stored layer and the output agree across the four tiles and across MODE 1 / MODE 2 (the sliced order), and
   across the four tiles under k_slices = 0 (the one-chain order).  Without forcing, frame i alone gives row i of the batch on
   every stored layer.
c. Integer-exact (cfg(bn=False), f32_probes.int_setup): all sums are integers below 2^24, so every summation order is exact
   and the stored output of the conv under test must EQUAL the integer reference followed by the epilogue restated in numpy
   float32 (bias add, v > 0 ? v : v * 0.1f, shortcut add), for all twelve plans; the raw w / h columns of the TRAIN=True
   output equal the head's sums restated from the stored output (two entries of +-1 per head row: one float32 addition in any
   K order, then the bias add).  SiLU has expf in it and cannot be restated bit for bit: k_tail_silu's twelve plans must
   agree bit for bit with each other and lie within 2^-22 relative of v / (1 + exp(-v)) evaluated in float64 (expf 1 ulp =
   2^-23, the add and the correctly rounded division 2^-24 each), results below the smallest normal float aside, and -0 from
   v = -89 down, where expf(-v) exceeds the largest float.
d. Floats (BatchNorm form, synthetic weights), once per K order, on the conv under test and every other stored conv:
   * worst case, leaky and linear probes:  |got - model| <= ((K + S + 2) u + 2^-52) D,  u = 2^-24, K = k k cin_p the chain
     length, S the number of slices (0: one chain), D = conv(|a|, |w s|) + |bias| + |shortcut operand|.  The terms: the model
     folds BatchNorm in double and the plan rounds the folded weight to float32 once (1 u on every product); a product enters
     a chain of at most K fused multiply-adds, each of which rounds once (K u); the S slice sums are added one after the other
     (at most S u); the float32 bias is added with one rounding (1 u); 2^-52 covers the model's own float64 arithmetic.  The
     leaky product and the shortcut add round once more each on the value; the formula does not name them, the measured
     maxima (below) stay under 7 u where the formula gives 38 u or more.  No fitted constant.
   * the project's layer-local gate unchanged: f16s3_emulation.gate(residual(got, rec), floors(rec)), rms and max of
     (value - model) / D at most GATE_M = 4 x the largest rms / max over three float32 evaluations on the CPU (torch NCHW,
     torch channels_last, 32-wide K chunks in the kernel's K order and slices).
   The decoded output passes the existing 1e-4 gate against the oracle (rect_ref.forward_rect).

Every test prints one "GATE ..." line per layer; profiles/experiments/f32_layer_local.log is one run's output.  Measured on an
MI355X, conv under test, sliced order | one-chain order, as rms / F_rms, max / F_max (and max |got - model| / D in u):

    m_tail         0.59, 0.53 (2.9 u) | 1.00, 0.92 (5.0 u)
    one_row        0.77, 0.57 (3.4 u) | 0.99, 1.00 (5.9 u)
    tiny_m         0.46, 0.44 (1.4 u) | 0.72, 0.55 (1.8 u)
    n_tail         1.00, 1.00 (4.6 u)
    k_tail         1.01, 1.07 (4.9 u)
    k_tail_sliced  0.49, 0.49 (2.1 u) | 1.00, 1.01 (4.4 u)
    ks4            0.54, 0.52 (2.4 u) | 0.99, 1.14 (5.2 u)
    ks4_shortcut   0.54, 0.40 (1.9 u) | 0.99, 1.12 (5.3 u)
    ks_pw          0.59, 0.43 (1.9 u) | 0.99, 1.11 (5.0 u)
    s2_odd         0.63, 0.44 (2.0 u) | 0.98, 0.96 (4.3 u)
    s2_even        0.48, 0.44 (2.0 u) | 1.00, 1.07 (4.9 u)
    big_map        1.00, 1.11 (4.8 u)
    stem_generic   1.01, 1.22 (3.3 u)
    k_tail_silu    1.00, 0.92 (5.6 u)
    k_tail_linear  1.00, 0.85 (5.0 u)
    concat_c64     0.57, 0.38 (1.9 u) | 1.00, 0.98 (4.8 u)

Worst over every stored conv of every probe (stems and 1x1 convs in front included): 1.01 F_rms, 1.22 F_max, 6.3 u.
"""
import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import cfgs
from f16_emulation import rel
from f16s3_emulation import floors, gate, residual, rms_max
from f32_probes import (BY_NAME, NAMES, PROBES, SCHEDULES, TILES, U, conv_launch, conv_records, epilogue_f32, expected_id,
                        expected_slices, head_train_columns, int_setup, setup, worst_case_bound)
from rect_ref import forward_rect
from test_narrow_gpu import _materialised

pytestmark = pytest.mark.gpu

TOL = 1e-4
_ids_run = {}                                        # probe name -> ids launch_infos() reported over its twelve plans


def _model(p, d, wts, bn=True, options=None):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(str(d / "net.cfg"), p.cfg(bn)), True).eval()
    m.net_info["height"] = p.in_h
    if p.in_w != p.in_h:
        m.input_width = p.in_w
    m.precision = "fp32"
    m.options = dict(options or {})
    m.keep_all_layers = True
    m.autotune = False
    m.load_weight_stream(wts)
    return m


def _stored(m, B):
    torch.cuda.synchronize()
    return {D["index"]: m.read_layer(D["index"], B).cpu() for D in _materialised(m)}


def _twelve(p, d, wts, bn=True):
    """(tile, schedule name, mode, model) of the twelve plans, prepared; the reported id is asserted (a)."""
    L = setup(p)[0].ir.layers[p.conv_layer]
    ids = set()
    for tile in TILES:
        for sched, opts, mode in SCHEDULES:
            m = _model(p, d, wts, bn, {"force_f32_variant": tile, **opts})
            m.prepare(p.B, torch.device("cuda", torch.cuda.current_device()))
            li = conv_launch(m.launch_infos(), p.conv_layer)
            assert li.variant == expected_id(L, tile, mode), (p.name, tile, sched, li.variant)
            ids.add(li.variant)
            yield tile, sched, mode, m
    _ids_run[p.name] = ids


def _same(tag, got, want):
    assert torch.equal(got[0], want[0]), (tag, "output")
    assert got[1].keys() == want[1].keys()
    for i, t in got[1].items():
        assert torch.equal(t, want[1][i]), (tag, "layer", i)


def _gate_layers(tag, ref, p, x, stored, sliced):
    """(d) on every stored conv of the probe; -> {stored layer: (rms / F_rms, max / F_max, max |r| / u)}"""
    failed, out = [], {}
    for i, rec in sorted(conv_records(ref, p, stored, x, sliced).items()):
        L = ref.ir.layers[rec["conv"]]
        got = stored[i]
        assert torch.isfinite(got).all(), (tag, i)
        r = residual(got, rec)
        fl = floors(rec)
        ok, q_rms, q_max = gate(r, fl)
        inside = bool(L.silu) or bool(((got.double() - rec["model"]).abs() <= worst_case_bound(rec)).all())
        out[i] = (q_rms, q_max, rms_max(r)[1] / U)
        print("GATE %s layer %d conv %dx%d/%d Cin %d Cout %d map %dx%d K %d slices %d: rms/D %.3e (%.2f F_rms) max/D %.3e (%.2f F_max, %.2f u; bound %d u)%s%s"
              % (tag, i, L.size, L.size, L.stride, L.cin, L.cout, L.hout, L.wout, rec["K"], rec["S"], rms_max(r)[0], q_rms, rms_max(r)[1], q_max,
                 rms_max(r)[1] / U, rec["K"] + rec["S"] + 2, "" if ok else "  EXCEEDS THE GATE at %s" % (np.unravel_index(np.abs(r).argmax(), r.shape),),
                 "" if inside else "  EXCEEDS THE WORST-CASE BOUND"))
        if not (ok and inside):
            failed.append((i, q_rms, q_max, inside))
    assert not failed, "%s: layers outside a gate (layer, rms / F_rms, max / F_max, inside the worst-case bound): %s" % (tag, failed)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_probe_every_tile_and_schedule_same_bits_and_inside_the_gates(tmp_path_factory, name):
    p = BY_NAME[name]
    ref, wts, x = setup(p)
    xg = x.cuda()
    d = tmp_path_factory.mktemp("f32p")
    sliced_layer = expected_slices(ref.ir.layers[p.conv_layer]) > 0
    first = {}                                        # K order -> (output, stored layers) of the first plan that ran it
    for tile, sched, mode, m in _twelve(p, d, wts):
        with torch.no_grad():
            y = m(xg).cpu()
        got = (y, _stored(m, p.B))
        assert p.stored_layer in got[1] and m.active_precision == "fp32"
        order = "sliced" if (sliced_layer and mode) else "one_chain"
        if order not in first:
            first[order] = got
        _same((name, tile, sched), got, first[order])                                   # (b)
        del m
    assert set(first) == ({"sliced", "one_chain"} if sliced_layer else {"one_chain"})
    # (b) the heuristic's tile: frame i alone == row i of the batch, every stored layer; the bits of the forced plans
    m = _model(p, d, wts)
    with torch.no_grad():
        y = m(xg).cpu()
    batch = (y, _stored(m, p.B))
    _same((name, "heuristic"), batch, first["sliced" if sliced_layer else "one_chain"])
    for i in range(p.B):
        with torch.no_grad():
            yi = m(xg[i:i + 1]).cpu()
        one = _stored(m, 1)
        assert torch.equal(yi[0], y[i]), (name, "frame", i)
        for k, t in one.items():
            assert torch.equal(t[0], batch[1][k][i]), (name, "frame", i, "layer", k)
    # (d) once per K order
    print("PROBE %s (%s): conv under test layer %d, ids %s" % (name, p.note, p.conv_layer, sorted(_ids_run[name])))
    line = []
    for order in ("sliced", "one_chain"):
        if order in first:
            q = _gate_layers("probe %s %s" % (name, order), ref, p, x, first[order][1], order == "sliced")[p.stored_layer]
            line.append("%.2f, %.2f (%.1f u)" % q)
    print("TABLE %-14s %s" % (name, " | ".join(line)))
    with torch.no_grad():
        want = forward_rect(ref, x)
    for order, (yo, _) in first.items():
        e = rel(yo.numpy(), want.numpy())
        assert yo.shape == want.shape and e.max() <= TOL, f"{order}: max rel err {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


@pytest.mark.parametrize("name", NAMES)
def test_probe_integer_sums_are_exact_on_every_tile_and_schedule(tmp_path_factory, name):
    p = BY_NAME[name]
    s = int_setup(p)
    xg = s["x"].cuda()
    silu = p.act == "silu"
    if silu:
        v = s["raw"] + s["bias"].view(1, -1, 1, 1)
        v64 = v.numpy()
        want64 = (v / (1.0 + torch.exp(-v))).numpy()
        # v is an integer: from -89 down expf(-v) exceeds the largest float, the kernel's v / (1 + expf(-v)) is -0 and the true
        # value (below 89 / FLT_MAX) is what it is off by
        tol64 = 2.0 ** -22 * np.abs(want64) + 2.0 ** -126 + np.where(v64 <= -89, np.abs(want64), 0.0)
        first = None
    else:
        want = epilogue_f32(s["raw"], s["bias"], p.act, s["res"])
    for tile, sched, mode, m in _twelve(p, tmp_path_factory.mktemp("f32i"), s["wts"], bn=False):
        m.TRAIN = True
        with torch.no_grad():
            y = m(xg).cpu()
        got = _stored(m, p.B)[p.stored_layer]
        g = got.numpy()
        if silu:
            first = g if first is None else first
            assert np.array_equal(g, first), (name, tile, sched)
            err = np.abs(g.astype(np.float64) - want64)
            q = err / tol64
            print("SILU %s tile %d %s: max error / tolerance %.3f at v = %g" % (name, tile, sched, q.max(), v64[np.unravel_index(q.argmax(), q.shape)]))
            assert (err <= tol64).all(), (name, tile, sched)
        else:
            bad = np.argwhere(g != want)
            assert not len(bad), "%s tile %d %s: %d values differ from the integer reference, first at (frame, channel, y, x) %s: got %r, want %r" % (
                name, tile, sched, len(bad), tuple(bad[0]), g[tuple(bad[0])], want[tuple(bad[0])])
        cols = head_train_columns(s["ref"], p, got)
        yc = y.numpy()[:, :, 2:4]
        bad = np.argwhere(yc != cols)
        assert yc.shape == cols.shape and not len(bad), "%s tile %d %s: head w / h columns differ at (frame, row, column) %s" % (name, tile, sched, tuple(bad[0]))
        del m


def test_the_probes_run_all_twelve_instantiations(tmp_path_factory):
    ids = set()
    for p in PROBES:
        if p.name not in _ids_run:                    # (run alone: prepare the plans, launch nothing)
            for _ in _twelve(p, tmp_path_factory.mktemp("f32a"), setup(p)[1]):
                pass
        ids |= _ids_run[p.name]
    assert ids == {tile + 10 * mode for tile in TILES for mode in (0, 1, 2)}, sorted(ids)
