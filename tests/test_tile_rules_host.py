"""CPU gate of the split-f16 tile rules (csrc/split_tiles.cpp, csrc/plan_tiles.cpp: Plan::tile_legal / default_tile / variant_for / set_tiles): the
whole matrix of forced ids 0 .. 169 and single-entry tile tables 0 .. 169, per launch, at batch 1 and 8, over every case of
tools/dump_tile_rules.py (cfgs x option sets x precisions 1 / 2), must be what tests/golden/tile_rules.json recorded: one
SHA-256 of the tool's printed text per case and the case's launch count.  On a mismatch run the tool for that case
(`python tools/dump_tile_rules.py --case NAME`) on both builds and diff the text: it names the launch and the id."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_tile_rules", os.path.join(ROOT, "tools", "dump_tile_rules.py"))
dump_tile_rules = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_tile_rules)

with open(os.path.join(ROOT, "tests", "golden", "tile_rules.json")) as _f:
    GOLDEN = json.load(_f)
CASES = {c[0]: c[1:] for c in dump_tile_rules.cases()}


def test_the_golden_file_covers_every_case():
    assert sorted(GOLDEN) == sorted(CASES) and len(CASES) == 10 * 8 * 2
    assert sum(1 for g in GOLDEN.values() if g["launches"] > 0) >= 120       # (the rest: plans the library refuses, recorded as such)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_and_installable_tiles_are_the_recorded_ones(name):
    assert dump_tile_rules.case_digest(*CASES[name]) == GOLDEN[name]
