"""The beam-search entries return the statuses they always did: the grid of tests/beam_status_grid.py against what the commit named in
tests/golden/beam_status_grid.json returned (tools/dev/beam_status_record.py).  No GPU: no call reaches HIP."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_status_grid as G  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_status_grid.json")
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert len(doc["commit"]) == 40
    return doc["statuses"]


@pytest.mark.parametrize("entry", list(G.ENTRIES))
def test_statuses_are_the_recorded_ones(entry, recorded):
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    want = recorded[entry]
    grid = G.cases(entry)
    assert [label for label, _ in grid] == list(want)              # the grid is the recorded one, case for case
    got = {label: G.status(lib, entry, ov) for label, ov in grid}
    assert {k: (got[k], want[k]) for k in got if got[k] != want[k]} == {}
    assert set(want.values()) >= {INVALID, WORKSPACE, UNSUPPORTED} and OK not in want.values()


def test_the_grid_has_what_it_should(recorded):
    assert set(recorded) == set(G.ENTRIES) and sum(len(v) for v in recorded.values()) > 1500
    for entry in G.ENTRIES:
        labels = set(recorded[entry])
        assert {"base", "lp=False", "T=0", "beam=-1", "ws='short'"} <= labels and sum(l.startswith("flags=") for l in labels) >= 63
        assert recorded[entry]["base"] == (INVALID if entry == "pgasr_ctc_beam_search_wide_lm" else WORKSPACE)
        assert recorded[entry]["ws='short'"] in (WORKSPACE, INVALID)
        T, beam = G._node_limit(entry)
        assert recorded[entry][f"T={T},beam={beam}"] == recorded[entry]["base"]      # no workspace: that refusal comes first


@pytest.mark.parametrize("entry", G.NARROW)
def test_lds_refusal_touches_no_device(entry):
    """beam 128 at V = 64 needs more LDS than a workgroup has: PGASR_ERR_UNSUPPORTED from every narrow entry, with a full-size workspace
    in HOST memory -- the refusal comes before the hash table is cleared.  (Not in the recorded grid: the 1-best entries used to clear
    the table first.)"""
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    ov = dict(T=2, B=1, V=64, beam=128, ws="full", nbest=3)
    assert G.status(lib, entry, ov) == UNSUPPORTED
    assert G.status(lib, entry, dict(ov, ws="short")) == WORKSPACE                    # the workspace is still checked first
    assert G.status(lib, entry, dict(ov, is_f64=1)) == UNSUPPORTED
    if G.ENTRIES[entry][2]:
        lm = dict(lm_table=True, lm_order=2, lm_alpha=0.5, lm_beta=0.1)
        assert G.status(lib, entry, dict(ov, **lm)) == UNSUPPORTED
        assert G.status(lib, entry, dict(ov, flags=16, **lm)) == UNSUPPORTED
    if G.ENTRIES[entry][3]:
        assert G.status(lib, entry, dict(ov, bias_table=True, bias_states=4, bias_weight=1.5)) == UNSUPPORTED
