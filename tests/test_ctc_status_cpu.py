"""The CTC loss section's entries return the statuses, and its size queries the sizes, they always did: the grid of
tests/ctc_status_grid.py against what the commit named in tests/golden/ctc_status_grid.json returned
(tools/dev/ctc_status_record.py).  No GPU: no call reaches HIP."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_status_grid as G  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_status_grid.json")
OK, INVALID, LAUNCH, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert len(doc["commit"]) == 40
    return doc


@pytest.mark.parametrize("entry", list(G.ENTRIES))
def test_statuses_are_the_recorded_ones(entry, recorded):
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    want = recorded["statuses"][entry]
    grid = G.cases(entry)
    assert [label for label, _ in grid] == list(want)              # the grid is the recorded one, case for case
    got = {label: G.status(lib, entry, ov) for label, ov in grid}
    assert {k: (got[k], want[k]) for k in got if got[k] != want[k]} == {}
    assert set(want.values()) == {INVALID, WORKSPACE, UNSUPPORTED}      # all three appear; PGASR_OK and a launch never do


@pytest.mark.parametrize("name", G.SIZES)
def test_sizes_are_the_recorded_ones(name, recorded):
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    want = recorded["sizes"][name]
    rows = G.size_cases()[name]
    assert [label for label, _ in rows] == list(want)
    got = {label: int(getattr(lib, name)(*args)) for label, args in rows}
    assert got == want
    assert want["base"] > 0 and want["T=0"] == 0 and 0 in want.values()


def test_the_grid_has_what_it_should(recorded):
    st = recorded["statuses"]
    assert set(st) == set(G.ENTRIES) and set(recorded["sizes"]) == set(G.SIZES) and sum(len(v) for v in st.values()) > 750
    assert len(G.GRADIENTS) == 14 and len(G.ENTRIES) == 18
    for entry, (kind, vmax, ntail) in G.ENTRIES.items():
        labels = set(st[entry])
        assert {"base", "lp=False", "T=0", "B=-1", "V=0", "blank=-1", f"V={vmax}", f"V={vmax + 1}", f"V={vmax + 1},lp=False"} <= labels
        assert st[entry]["base"] == WORKSPACE and st[entry][f"V={vmax}"] == WORKSPACE and st[entry][f"V={vmax + 1}"] == UNSUPPORTED
        assert st[entry][f"V={vmax + 1},lp=False"] == INVALID and st[entry][f"V={vmax + 1},blank=-1"] == INVALID
        if kind in ("seq", "nbest"):
            assert st[entry]["hws='short',ws='full'"] == WORKSPACE and st[entry]["ws='full'"] == WORKSPACE
            assert st[entry]["K=17,Lmax=-1"] == INVALID and st[entry]["Lh=1024,Lmax=1024"] == UNSUPPORTED
            assert st[entry]["B=33554432,K=16"] == UNSUPPORTED
        if kind in ("multi", "seq", "nbest"):
            assert st[entry]["K=0"] == INVALID and st[entry]["K=17"] == INVALID and st[entry]["K=16"] == WORKSPACE
            assert st[entry][f"K=0,V={vmax + 1}"] == INVALID
        if ntail == 3:
            assert st[entry]["ref=True"] == INVALID and st[entry]["kl=True"] == INVALID and st[entry]["ent=True"] == WORKSPACE
            assert st[entry]["kl=True,ref=True"] == WORKSPACE
    wide_nbest = st["pgasr_ctc_grad_from_lattices_seq_wide"]
    assert wide_nbest["pg_paths=False"] == WORKSPACE and wide_nbest["ent=True,pg_paths=False"] == INVALID
    assert wide_nbest["kl=True,pg_paths=False,ref=True"] == INVALID
