"""Every beam-search call of tests/beam_dispatch_calls.py returns, word for word, what the commit named in
tests/golden/beam_dispatch_parent.npz returned for it on the MI355X (tools/dev/beam_dispatch_record.py): the host dispatch picks the
kernel, the instantiation and the argument tail it always did."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_dispatch_calls as D  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_dispatch_parent.npz")


@pytest.mark.gpu
def test_every_call_returns_the_recorded_words():
    with np.load(GOLDEN) as doc:
        assert len(str(doc["commit"])) == 40
        want = D.unpack(doc)
    got = D.run_all()
    assert sorted(got) == sorted(want) and len(got) > 380
    kinds = {n.split("-")[0] for n in got}
    assert kinds == {"best", "list", "raw", "wide"}
    assert [n for n in got if got[n] != want[n]] == []
    # the matrix separates what it should: an LM, a bias, the list and the exact path each change the words of some call
    assert want["best-V29-f32-K4-nolm-nobias-c0g0l0"] != want["best-V29-f32-K4-lm-nobias-c0g0l0"]
    assert want["wide-f32-n3-lm1-bias1-c0"] != want["wide-f64-n3-lm1-bias1-c0"]
    assert want["raw-V40-f32-K4-flags0"] == want["best-V40-f32-K4-nolm-nobias-c0g0l0"]
    # beam 17 is outside the single-wave kernel: its flags change nothing there
    assert want["best-V29-f32-K17-nolm-nobias-c0g0l0"] == want["best-V29-f32-K17-nolm-nobias-c0g1l1"]
    assert want["list-V29-f32-K17-lm-nobias-c0f0l0"] == want["list-V29-f32-K17-lm-nobias-c0f1l1"]
