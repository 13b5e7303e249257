"""CPU tests of the float64 model of the split-f16 format (tests/f16s3_emulation.py), of the layer-local gate the GPU tests
apply (tests/test_f16s3_local_gpu.py) and of the probe networks (tests/conv_probes.py).

* The walk: with the planes switched off (rounding=False) the model is the oracle's graph evaluated in float64; with all FOUR
  product terms and no store rounding each layer lies within the representation error of the planes of it.
* The table: per probe and stored conv layer, the distances (per element, in units of D = conv(|a|, |w|) + |bias| + |shortcut|)
  of the model to the exact float64 conv, of the three float32 reference evaluations to the model, and of each mutant.
* Teeth: every mutant of f16s3_emulation.MUTANTS, applied to the conv under test of every probe in which it is applicable,
  must FAIL gate() at its m = 4.  A mutant that passes means the gate is too loose for that shape.
* Coverage: over all probes, the tile ids rtod_plan_set_tiles accepts for the convs under test are every id of every family.
"""
import pytest
import torch

from rect_ref import forward_rect
from conv_probes import FAMILIES, PROBES, BY_NAME, legal_ids, setup
from f16s3_emulation import F16S3Emulation, GATE_M, MUTANTS, floors, gate, residual, rms_max

NAMES = [p.name for p in PROBES]


class _Ref64:
    """The oracle's graph and parameters in float64."""

    def __init__(self, ref):
        self.ir, self.height = ref.ir, ref.height
        self.params = {i: {k: v.double() for k, v in p.items()} for i, p in ref.params.items()}


_base = {}


def _baseline(p):
    """Model, D and the float32 reference evaluations of every stored conv layer of a probe (cumulative: no feed), once."""
    if p.name not in _base:
        ref, _, x = setup(p)
        emu = F16S3Emulation(ref, p.options)
        with torch.no_grad():
            y, layers, recs = emu.forward(x, keep_layers=True, records=True, references=True)
        _base[p.name] = (emu, y, layers, recs)
    return _base[p.name]


def applicable(mutant, p):
    return p.shortcut if mutant == "shortcut_lo" else True


@pytest.mark.parametrize("name", ["w33_c96_shortcut", "w33_c96_silu", "s2_c64", "narrow_c16", "ks_pw_c256"])
def test_without_planes_the_walk_is_the_oracle_in_float64(name):
    p = BY_NAME[name]
    ref, _, x = setup(p)
    emu = F16S3Emulation(ref, p.options)
    with torch.no_grad():
        want, outs = forward_rect(_Ref64(ref), x.double(), keep_layers=True)
        y0, l0 = emu.forward(x, rounding=False, keep_layers=True)
        # float64 rounding only: conv -> batch_norm -> activation against the folded conv, ~1e-15 per operation
        assert float(((y0 - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-12
        stored = [i for i, t in l0.items() if t is not None]
        assert len(stored) >= len(ref.ir.layers) - 2
        for i in stored:
            assert float((l0[i] - outs[i]).abs().max()) <= 1e-12 * max(1.0, float(outs[i].abs().max())), i
        # all four product terms, no store rounding, every layer from the oracle's float64 inputs: what is left is the
        # representation error of the operands.  hi + lo carries 22 bits (2^-22 relative per operand, worst case), the folded
        # weight is a float32 (2^-24): 2^-22 + 2^-22 + 2^-24 < 2^-20 per product, summed against D
        feed = {i: outs[i] for i in stored}
        _, l4, recs = emu.forward(x, all_terms=True, store_rounding=False, keep_layers=True, feed=feed, records=True)
        assert p.stored_layer in recs
        for i, rec in recs.items():
            r = ((l4[i] - outs[i]) / rec["D"]).abs()
            assert float(r.max()) <= 2.0 ** -20, (i, float(r.max()))


@pytest.mark.parametrize("name", NAMES)
def test_table_of_floors_and_mutants_and_every_mutant_fails_the_gate(name):
    p = BY_NAME[name]
    emu, _, layers, recs = _baseline(p)
    _, _, x = setup(p)
    assert p.stored_layer in recs and recs[p.stored_layer]["conv"] == p.conv_layer
    print("probe %s: %s" % (p.name, p.note))
    for i, rec in sorted(recs.items()):
        L = emu.ir.layers[rec["conv"]]
        print("  layer %d (conv %d: %dx%d, Cin %d, Cout %d, stride %d, K slices of %d chunks)"
              % (i, rec["conv"], L.size, L.size, L.cin, L.cout, L.stride, rec["k_slices"]))
        print("    %-28s rms/D %.2e  max/D %.2e" % (("model vs exact float64",) + rms_max(residual(rec["exact"], rec))))
        for k, v in rec["refs"].items():
            print("    %-28s rms/D %.2e  max/D %.2e" % (("float32 " + k + " vs model",) + rms_max(residual(v, rec))))
    rec = recs[p.stored_layer]
    fl = floors(rec)
    print("  floors of the conv under test: F_rms %.2e, F_max %.2e; gate at m = %g" % (fl + (GATE_M,)))
    # the references themselves pass, and so does the exact float64 conv: the format's own error lies under the float32 floor
    for k, v in list(rec["refs"].items()) + [("exact", rec["exact"])]:
        assert gate(residual(v, rec), fl)[0], k
    feed = {i: t for i, t in layers.items() if t is not None and i != p.stored_layer}
    passed = []
    for mutant in MUTANTS:
        if not applicable(mutant, p):
            continue
        with torch.no_grad():
            _, lm = emu.forward(x, keep_layers=True, feed=feed, mutant=(mutant, p.conv_layer))
        r = residual(lm[p.stored_layer], rec)
        ok, q_rms, q_max = gate(r, fl)
        print("    mutant %-24s rms/D %.2e (%.1f x F_rms)  max/D %.2e (%.1f x F_max)%s"
              % ((mutant,) + (rms_max(r)[0], q_rms, rms_max(r)[1], q_max) + ("   PASSES THE GATE" if ok else "",)))
        if ok:
            passed.append(mutant)
    assert not passed, "the gate is too loose for %s: %s" % (p.name, passed)


def test_the_probes_reach_every_tile_of_every_family():
    reached = set()
    for p in PROBES:
        ids = legal_ids(p, 1)
        assert ids, p.name
        f16 = legal_ids(p, 2)
        assert f16 and set(f16) <= set(ids), p.name                          # plain f16: a subset, never empty
        reached |= set(ids)
    every = set()
    for r in FAMILIES.values():
        every |= set(r)
    assert every == (set(range(0, 12)) | set(range(50, 78)) | set(range(90, 101)) | set(range(110, 115)) | set(range(140, 144)) |
                     set(range(150, 156)))
    assert reached == every, "tiles that only whole networks exercise: %s" % sorted(every - reached)


def test_the_probes_reach_the_corners_they_are_there_for():
    ids = {p.name: set(legal_ids(p, 1)) for p in PROBES}
    lds_band, two_group = {50, 51, 52, 53, 54, 55, 56, 61, 62, 63, 66}, {57, 58, 59, 60, 64, 65, 67, 69}
    for n in ("w94_c32", "w94_one_row", "w94_c96", "w33_c96", "w33_c96_shortcut", "w33_c96_silu", "w33_c96_linear", "hw420_c512"):
        assert ids[n] == lds_band, n
    assert ids["hw400_c512"] == two_group
    assert 68 in ids["w95_c32"] and 68 in ids["w160_c32"] and 68 not in ids["w161_c32"] and 68 not in ids["w94_c32"]
    assert set(range(110, 115)) <= ids["w95_c32"] and set(range(110, 115)) <= ids["w161_c32"]
    assert set(range(110, 114)) <= ids["w160_c32"] and 114 not in ids["w160_c32"]
    for n in ("slab_c64", "slab_c192"):
        assert set(range(90, 101)) <= ids[n], n
    for n in ("pw_c96", "s2_c64"):
        assert ids[n] == set(range(0, 12)) | set(range(70, 78)), n
    assert ids["narrow_c16"] == set(range(140, 144))
    assert ids["ks_pw_c256"] == ids["ks_c64"] == set(range(150, 156))
