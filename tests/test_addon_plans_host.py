"""The add-on units' host-only `*_workspace_bytes` and `*_plan` exports against tests/golden/addon_plans.json, number for number: a
workspace layout is written once, in plan(), and every offset behind a size is what a launcher hands to a kernel, so a byte of drift is
memory corruption on the device.  The fixture (oracle/make_addon_plans.py, which also holds the table and says what it covers) was
recorded from the library before the layouts moved to csrc/ws_layout.h.  No device is needed."""
import json
import os

import pytest

from oracle import make_addon_plans as M
from stego_amd import capi

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "addon_plans.json")) as f:
    ROWS = json.load(f)


def test_fixture_holds_the_table():
    """every row of the generator's table is in the fixture, in order, and every function has rows"""
    assert [(r["fn"], r["args"]) for r in ROWS] == [(fn, args) for fn, args in M.table()]
    assert {r["fn"] for r in ROWS} == set(M.FUNCS)
    assert len(ROWS) >= 300


@pytest.mark.parametrize("fn", sorted(M.FUNCS))
def test_plans_and_workspace_sizes_match_the_fixture(fn):
    rows = [r for r in ROWS if r["fn"] == fn]
    bad = []
    for r in rows:
        got = M.evaluate(capi, fn, r["args"])
        if got != {"ws": r["ws"], "plan": r["plan"]}:
            bad.append((r["args"], got, {"ws": r["ws"], "plan": r["plan"]}))
    assert not bad, "%d of %d rows differ, first (args, got, recorded): %r" % (len(bad), len(rows), bad[0])
    # the table reaches both answers: descriptors the unit plans for and descriptors it refuses
    sizes = [r["ws"] if r["ws"] is not None else r["plan"][0] for r in rows]
    assert any(sizes) and not all(sizes)
