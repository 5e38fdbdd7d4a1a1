"""Every gradient, loss and hypothesis-lattice call of tests/ctc_dispatch_calls.py returns, bit for bit, what the commit named in
tests/golden/ctc_dispatch_parent.npz returned for it on the MI355X (tools/dev/ctc_dispatch_record.py): the host dispatch and the
Python call path pick the entry, the kernel family, the instantiation and the argument tail they always did."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_dispatch_calls as D  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_dispatch_parent.npz")


@pytest.mark.gpu
def test_every_call_returns_the_recorded_words():
    with np.load(GOLDEN) as doc:
        assert len(str(doc["commit"])) == 40
        want = D.unpack(doc)
    got = D.run_all()
    for name in sorted(got):
        print(name, got[name][:16], "" if got[name] == want.get(name) else "  <-- recorded " + str(want.get(name))[:16])
    assert sorted(got) == sorted(want) and len(got) > 300          # the set of calls is the recorded one
    assert {n.split("-")[0] for n in got} == {"loss", "lattice", "one", "multi", "steps", "stepsconst", "hyp", "seq", "nbest", "raw"}
    assert [n for n in got if got[n] != want[n]] == []
    for V, wide in [(v, False) for v in D.NARROW_V] + [(v, True) for v in D.WIDE_V]:
        tag = f"{'wide' if wide else 'narrow'}-V{V}"
        # a tail changes the digest of the same call without it, and the tails differ from each other
        forms = ["multi", "steps", "seq"] + ([] if wide else ["one-utt", "one-nopg", "one-frame"])
        for form in forms:
            kind, _, sub = form.partition("-")
            four = [want[f"{kind}-{tag}-{sub + '-' if sub else ''}{tail}"] for tail in D.TAILS]
            assert len(set(four)) == 4, (form, tag)
        # per-frame coefficients that are constant over t give the per-utterance digest
        for tail in D.TAILS if not wide else D.TAILS[:1]:
            assert want[f"one-{tag}-frameconst-{tail}"] == want[f"one-{tag}-utt-{tail}"] != want[f"one-{tag}-frame-{tail}"]
            assert want[f"one-{tag}-nopg-{tail}"] != want[f"one-{tag}-utt-{tail}"]
        for tail in D.TAILS:
            assert want[f"stepsconst-{tag}-{tail}"] == want[f"multi-{tag}-{tail}"] != want[f"steps-{tag}-{tail}"]
            assert want[f"seq-{tag}-{tail}"] != want[f"multi-{tag}-{tail}"]
        assert want[f"nbest-{tag}-none"] != want[f"seq-{tag}-none"] and want[f"hyp-{tag}-nbest"] != want[f"hyp-{tag}-seq"]
        assert want[f"loss-{tag}-grad"] != want[f"loss-{tag}-nograd"]
        if not wide:        # the forwarding chain: NULL tails are the entry without them
            for form, plain in (("one", f"one-{tag}-utt"), ("multi", f"multi-{tag}"), ("seq", f"seq-{tag}")):
                assert want[f"raw-{tag}-{form}_ent-null"] == want[f"raw-{tag}-{form}_kl-null"] == want[f"{plain}-none"]
                assert want[f"raw-{tag}-{form}_kl-ent"] == want[f"{plain}-ent"]
