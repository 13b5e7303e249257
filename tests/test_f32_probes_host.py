"""CPU tests of the probes for the exact-fp32 conv kernel (tests/f32_probes.py) and of the gates tests/test_f32_probes_gpu.py
applies.  No device.

* The plan: for every probe and every ``force_f32_variant`` 0..3, through the C ABI at precision 0, the conv under test is a
  kind-0 launch whose reported variant % 10 is the forced tile, it is reported as sliced (variant // 10 >= 1) exactly where
  ``expected_slices`` says so, and never under option ``k_slices = 0``.  Over all probes both K orders occur.
* The integer form: sum |w| |x| < 2^24 in every conv in front of the head (asserted inside ``int_setup``), the oracle in
  float32 reproduces the integer reference exactly, the restated epilogue is the oracle's.
* Teeth: torch's float32 conv, judged as the value, passes f16s3_emulation.gate (m = 4) and the worst-case bound on every
  probe, from the oracle's stored inputs; every mutant of f32_probes.MUTANTS fails the gate on every probe where it applies,
  in the K order the default plan runs and in the one-chain order.
"""
import numpy as np
import pytest
import torch

from rect_ref import forward_rect
from f16s3_emulation import GATE_M, floors, gate, residual, rms_max
from f32_probes import (BY_NAME, MUTANTS, NAMES, PROBES, TILES, applicable, conv_launch, conv_record, conv_records, epilogue_f32,
                        expected_id, expected_slices, host_plan, int_setup, k_dims, n_slices, setup, value_f32, worst_case_bound)


def _launch(p, options):
    plan = host_plan(p, options)
    try:
        return conv_launch(plan.launches(), p.conv_layer)
    finally:
        plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_forced_tile_and_slicing_are_what_the_plan_reports(name):
    p = BY_NAME[name]
    L = setup(p)[0].ir.layers[p.conv_layer]
    assert (L.hin, L.win, L.cin, L.cout, L.size, L.stride) == (p.H, p.W, p.cin, p.cout, p.k, p.stride)
    for tile in TILES:
        li = _launch(p, (("force_f32_variant", tile),))
        assert li.kind == 0 and li.variant % 10 == tile, (name, tile, li.variant)
        assert (li.variant // 10 >= 1) == (expected_slices(L) > 0), (name, tile, li.variant)
        assert li.variant == expected_id(L, tile, 1)              # no device: no scratch, the in-workgroup schedule
        li = _launch(p, (("force_f32_variant", tile), ("k_slices", 0)))
        assert li.variant == tile, (name, tile, li.variant)
        li = _launch(p, (("force_f32_variant", tile), ("k_slice_workgroups", 0)))
        assert li.variant == expected_id(L, tile, 1)


def test_the_probes_reach_the_shapes_they_are_there_for():
    dims = {p.name: k_dims(setup(p)[0].ir.layers[p.conv_layer]) for p in PROBES}
    sl = {p.name: (expected_slices(setup(p)[0].ir.layers[p.conv_layer]), n_slices(setup(p)[0].ir.layers[p.conv_layer])) for p in PROBES}
    assert sl["m_tail"] == sl["one_row"] == sl["tiny_m"] == sl["s2_odd"] == (2, 5)            # 9 chunks: 2,2,2,2,1
    assert dims["k_tail_sliced"] == (120, 1080, 1088) and sl["k_tail_sliced"] == (9, 4)       # 34 chunks: 9,9,9,7
    assert sl["ks4"] == sl["ks4_shortcut"] == sl["s2_even"] == sl["concat_c64"] == (4, 5)     # 18 chunks: 4,4,4,4,2
    assert sl["ks_pw"] == (2, 4)
    assert dims["k_tail"] == (20, 180, 192) and dims["stem_generic"] == (4, 36, 64)
    for n in ("n_tail", "k_tail", "k_tail_silu", "k_tail_linear", "big_map", "stem_generic"):
        assert sl[n] == (0, 0), n
    big = setup(BY_NAME["big_map"])[0].ir.layers[BY_NAME["big_map"].conv_layer]
    assert big.hout * big.wout == 2809 and k_dims(big)[2] // 32 >= 8                           # unsliced by the map rule alone
    # without forcing: the heuristic's tile, which depends on Cout and, above 64 filters, on the batch
    assert _launch(BY_NAME["big_map"], ()).variant % 10 == 3 and _launch(BY_NAME["m_tail"], ()).variant % 10 == 1


@pytest.mark.parametrize("name", NAMES)
def test_integer_form_is_exact_in_float32(name):
    p = BY_NAME[name]
    s = int_setup(p)                                               # asserts sum |w| |x| < 2^24 per conv
    assert set(s["absum"]) == {L.index for L in s["ref"].ir.layers[:p.conv_layer + 1] if L.type == "convolutional"}
    print("probe %s: max sum |w||x| per conv %s" % (name, s["absum"]))
    with torch.no_grad():
        _, outs = forward_rect(s["ref"], s["x"], keep_layers=True)
    if p.act == "silu":
        return
    want = epilogue_f32(s["raw"], s["bias"], p.act, s["res"])
    assert np.array_equal(outs[p.stored_layer].numpy(), want), name
    assert (want < 0).any() or p.act != "leaky"                    # the slope is exercised


_base = {}


def _baseline(p):
    if p.name not in _base:
        ref, _, x = setup(p)
        with torch.no_grad():
            _, outs = forward_rect(ref, x, keep_layers=True)
        _base[p.name] = (ref, x, outs)
    return _base[p.name]


@pytest.mark.parametrize("name", NAMES)
def test_torch_float32_passes_the_gates_and_every_mutant_fails(name):
    p = BY_NAME[name]
    ref, x, outs = _baseline(p)
    L = ref.ir.layers[p.conv_layer]
    passed = []
    for sliced in (True, False):
        if not sliced and not expected_slices(L):
            continue
        rec = conv_record(ref, p, outs, x, sliced=sliced)
        fl = floors(rec)
        value = value_f32(ref, p, outs, x)
        ok, q_rms, q_max = gate(residual(value, rec), fl)
        print("probe %s (%s), K %d, %d slices: F_rms %.2e F_max %.2e; torch float32: %.2f F_rms, %.2f F_max; gate at m = %g"
              % (name, p.note, rec["K"], rec["S"], fl[0], fl[1], q_rms, q_max, GATE_M))
        assert ok, (name, q_rms, q_max)
        for k, v in rec["refs"].items():                           # every reference evaluation passes both gates
            assert gate(residual(v, rec), fl)[0], k
            if p.act != "silu":
                assert bool(((v - rec["model"]).abs() <= worst_case_bound(rec)).all()), k
        for mutant in MUTANTS:
            if not applicable(mutant, p, L):
                continue
            r = residual(value_f32(ref, p, outs, x, mutant), rec)
            ok, q_rms, q_max = gate(r, fl)
            print("    mutant %-16s rms/D %.2e (%.1f x F_rms)  max/D %.2e (%.1f x F_max)%s"
                  % ((mutant,) + (rms_max(r)[0], q_rms, rms_max(r)[1], q_max) + ("   PASSES THE GATE" if ok else "",)))
            if ok:
                passed.append((mutant, sliced))
    assert not passed, "the gate is too loose for %s: %s" % (name, passed)


def test_every_stored_conv_of_a_probe_has_a_record():
    for p in PROBES:
        ref, x, outs = _baseline(p)
        recs = conv_records(ref, p, outs, x)
        convs = [L.index for L in ref.ir.layers[:p.conv_layer + 1] if L.type == "convolutional"]
        assert sorted(r["conv"] for r in recs.values()) == convs and p.stored_layer in recs, p.name
        for i, rec in recs.items():
            assert rec["model"].shape == outs[i].shape and float(rec["D"].min()) > 0, (p.name, i)
