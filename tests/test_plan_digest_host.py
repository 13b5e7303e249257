"""CPU gate of what a plan is and what it uploads (the csrc/plan_*.cpp files: cfg, planning, weight packing, launch records): per
case of tools/dump_plan_digest.py (cfgs x option sets x precisions x keep_all_layers x weight sets) the packed weight image of
rtod_plan_pack_weights, the rtod_plan_describe text and the rtod_launch_info records at batch 8 and 1 must hash to what
tests/golden/plan_digest.json recorded; a refused plan must be refused for the recorded reason.  On a mismatch run the tool for
that case (`python tools/dump_plan_digest.py --case NAME`) on both builds and diff the text."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_plan_digest", os.path.join(ROOT, "tools", "dump_plan_digest.py"))
dump_plan_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plan_digest)

with open(os.path.join(ROOT, "tests", "golden", "plan_digest.json")) as _f:
    GOLDEN = json.load(_f)
CASES = {c[0]: c[1:6] for c in dump_plan_digest.cases()}


def test_the_golden_file_covers_every_case():
    assert sorted(GOLDEN) == sorted(CASES)
    refused = [n for n, g in GOLDEN.items() if "refused" in g]
    assert len(refused) == 7 and not any("?" in GOLDEN[n]["refused"] for n in refused)      # every refusal is of a known kind
    for n, g in GOLDEN.items():
        assert n in refused or (g["packed_floats"] > 0 and all(len(g[k]) == 64 for k in ("weights_sha256", "describe_sha256", "launches_sha256")))


def test_every_packing_branch_and_every_option_is_covered():
    branches, options = dump_plan_digest.coverage()
    assert all(branches[b] for b in dump_plan_digest.BRANCHES), branches
    assert all(options[o] for o in dump_plan_digest.OPTION_DEFAULTS), options
    for b, names in branches.items():                   # a case named for a branch really plans (or, for "refused", really is refused)
        assert all(("refused" in GOLDEN[n]) == (b == "refused") for n in names), b


def test_k_slices_split_changes_the_plan_but_not_the_image():
    a, b = GOLDEN["kslice_mini/defaults/p1/synth"], GOLDEN["kslice_mini/kslices/p1/synth"]
    assert a["weights_sha256"] == b["weights_sha256"] and a["packed_floats"] == b["packed_floats"]
    assert a["describe_sha256"] != b["describe_sha256"] and a["launches_sha256"] != b["launches_sha256"]


def test_the_edge_weights_change_the_image_alone():
    pairs = [n for n in CASES if n.endswith("/edge")]
    assert len(pairs) >= 20
    for n in pairs:
        e, s = GOLDEN[n], GOLDEN[n[:-len("edge")] + "synth"]
        assert e["weights_sha256"] != s["weights_sha256"]
        assert (e["describe_sha256"], e["launches_sha256"], e["packed_floats"]) == (s["describe_sha256"], s["launches_sha256"], s["packed_floats"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_and_packed_weights_are_the_recorded_ones(name):
    assert dump_plan_digest.case_digest(*CASES[name]) == GOLDEN[name]
