"""tests/confidence_ref.py, the statement csrc/confidence.hip is held to (include/pgasr_hip.h, A10-CONF), against hand-worked
numbers and its own invariants; the generated inputs of tests/test_confidence_gpu.py shown to be discriminating; and
metrics.confidence_nce against a direct numpy evaluation.  No GPU."""
import math

import numpy as np
import pytest

import confidence_cases as C
import confidence_ref as R
import editops_ref


def test_hand_worked_list():
    """Pivot "abc" against "abc", "abd", "ac", "xabcc" with weights 1/2, 1/4, 1/8, 1/8: the alignments are HHH, HHS, HDH and
    IHHIH, so position a has every row's mass, b all but "ac"'s, c all but "abd"'s; one insertion in front of a and one in front
    of c, each with 1/8."""
    rows, weights, want = C.hand_case()
    assert [editops_ref.edit_ops(list(rows[0]), list(r))[1] for r in rows] == [[0, 0, 0], [0, 0, 1], [0, 2, 0], [3, 0, 0, 3, 0]]
    conf, sub, dele, ins, left = R.nbest_confidence(rows, weights, 0)
    assert conf == want["conf"] and sub == want["substituted"] and dele == want["deleted"] and ins == want["inserted"]
    assert left == 0


def test_hand_worked_words_and_other_pivot():
    rows, weights, want = C.hand_case()
    words = [tuple(R.words_of(" ".join(r), " ")) for r in rows]
    assert words[3] == (("x",), ("a",), ("b",), ("c",), ("c",))
    conf, sub, dele, ins, _ = R.nbest_confidence(words, weights, 0)
    assert (conf, sub, dele, ins) == (want["conf"], want["substituted"], want["deleted"], want["inserted"])
    # pivot "ac": "abc" -> H I H, "abd" -> H I S, "ac" -> H H, "xabcc" -> I H I I H: five insertions in all, one substitution of c
    conf, sub, dele, ins, _ = R.nbest_confidence(rows, weights, 2)
    assert conf[0] == 1.0 and conf[1] + sub[1] + dele[1] == 1.0 and sub[1] == 0.25
    assert sum(ins) == 0.5 + 0.25 + 3 * 0.125


def test_sides_slots_and_left_out_by_hand():
    """side "hyp": slots are hypothesis positions, the insertion is the own gap operation and deletions fall into gaps.  A pair
    with another slot count is left out; non-participating weights are skipped and do not set n_slots."""
    lists = [[0, 3, 3, 2, 2, 1], [2, 2, 2, 0, 0, 0, 0], [0, 0, 0], [1, 1, 1, 1]]
    mass, n_slots, left = R.group_mass(lists, [float("nan"), 0.5, 0.25, 0.25], "hyp", 6)
    assert n_slots == 4 and left == 1                       # the NaN pair is no pivot; [0, 0, 0] has three slots
    assert mass[0] == [0.5, 0.5, 0.5, 0.5, 0, 0, 0] and mass[1] == [0.25] * 4 + [0, 0, 0] and mass[2] == [0.0] * 7
    assert mass[3] == [1.5, 0, 0, 0, 0, 0, 0]               # three deletions in front of position 0: one product 0.5 * 3
    mass, n_slots, left = R.group_mass(lists[:1], [0.5], "hyp", 6)
    assert n_slots == 4 and mass[0][:4] == [0.5, 0, 0, 0] and mass[2][:4] == [0, 0.5, 0.5, 0] and mass[1][:4] == [0, 0, 0, 0.5]
    assert mass[3][:5] == [0, 0, 0, 1.0, 0]
    mass, n_slots, left = R.group_mass(lists[:1], [0.5], "ref", 6)
    assert n_slots == 4 and mass[0][:4] == [0.5, 0, 0, 0] and mass[2][:4] == [0, 0.5, 0.5, 0] and mass[3][:5] == [0, 1.0, 0, 0, 0]
    # more slots than the output has: the pair is left out, the pivot's length is still reported
    mass, n_slots, left = R.group_mass(lists[:1], [0.5], "ref", 3)
    assert n_slots == 4 and left == 1 and all(x == 0 for ch in mass for x in ch)
    mass, n_slots, left = R.group_mass(lists, [0.0, -1.0, float("inf"), float("nan")], "ref", 6)
    assert n_slots == -1 and left == 0 and all(x == 0 for ch in mass for x in ch)


def _all_groups():
    for K, pivot, rows, weights, flags in C.length_cases():
        yield "K%d" % K, pivot, rows, weights, flags
    for pg, G, groups in C.shape_cases():
        for g, (pivot, rows, weights, flags) in enumerate(groups):
            yield "pg%d_G%d_g%d" % (pg, G, g), pivot, rows, weights, flags


def test_masses_add_up_and_sides_mirror():
    """On every generated group: hit + sub + gap at each slot is the participating weight (within 1e-12; the additions differ in
    order), and the mirrored operation strings under side "hyp" give side "ref"'s masses bit for bit."""
    for name, pivot, rows, weights, _ in _all_groups():
        n = len(pivot)
        lists = C.op_lists(pivot, rows, "ref")
        mass, n_slots, left = R.group_mass(lists, weights, "ref", n + 2)
        assert n_slots == n and left == 0, name
        total = math.fsum(weights)
        for i in range(n):
            assert abs(mass[0][i] + mass[1][i] + mass[2][i] - total) < 1e-12, name
        assert all(mass[ch][i] == 0 for ch in range(3) for i in range(n, n + 3)) and mass[3][n + 1] == mass[3][n + 2] == 0
        ins_total = math.fsum(w * sum(1 for o in ops if o == 3) for w, ops in zip(weights, lists))
        assert abs(math.fsum(mass[3]) - ins_total) < 1e-9, name
        mirrored = R.group_mass([C.mirror(o) for o in lists], weights, "hyp", n + 2)
        assert mirrored == (mass, n_slots, left), name
        # the swapped pairs themselves: another canonical alignment, the same total mass per slot
        mass_h, n_h, left_h = R.group_mass(C.op_lists(pivot, rows, "hyp"), weights, "hyp", n + 2)
        assert n_h == n and left_h == 0
        for i in range(n):
            assert abs(mass_h[0][i] + mass_h[1][i] + mass_h[2][i] - total) < 1e-12, name


def test_length_cases_hit_their_operation_counts():
    for K, pivot, rows, _, _ in C.length_cases():
        lens = [len(o) for o in C.op_lists(pivot, rows, "ref")]
        assert K in lens, (K, lens)
        assert K in [len(o) for o in C.op_lists(pivot, rows, "hyp")]


def test_the_inputs_are_discriminating():
    """At least half of the random pairs have more than one optimal alignment, so that the tie rule decides masses; every case has
    a pair with two or more insertions in one gap, so that a kernel that lets them meet in one cell is caught.  Ties are counted
    with count_optimal_alignments up to 300 symbols; above, by the equivalent test that the walk with the opposite preference
    leaves the canonical one (shown equivalent on the short pairs)."""
    tied = total = 0
    for name, pivot, rows, _, flags in _all_groups():
        runs = False
        for row, is_random in zip(rows, flags):
            ops = editops_ref.edit_ops(pivot, row)[1]
            runs = runs or C.has_run_of_other(ops, "ref")
            assert C.has_run_of_other(C.mirror(ops), "hyp") == C.has_run_of_other(ops, "ref")
            if not is_random:
                continue
            D = editops_ref.matrix(pivot, row)
            other_way = editops_ref.walk(pivot, row, D=D, order=("ins", "del", "diag")) != ops
            if len(pivot) <= 300 and total < 400:
                assert (editops_ref.count_optimal_alignments(pivot, row, D=D) > 1) == other_way
            tied += other_way; total += 1
        if len(pivot) + len(rows) > 1 and name != "K1":
            assert runs, name
    assert total >= 100 and 2 * tied >= total, (tied, total)


def test_batched_statement_matches_the_groups():
    pg, G, groups = C.shape_cases()[5]                       # 16 pairs, 5 groups
    lists = [o for pivot, rows, _, _ in groups for o in C.op_lists(pivot, rows, "ref")]
    weight = [w for _, _, ws, _ in groups for w in ws]
    ops, n_ops = C.pack_ops(lists)
    mass, n_slots, left = R.slot_mass(ops, n_ops, weight, pg, "ref", 80)
    for g, (pivot, rows, ws, _) in enumerate(groups):
        m, ns, lo = R.group_mass(C.op_lists(pivot, rows, "ref"), ws, "ref", 80)
        assert np.array_equal(mass[g], np.asarray(m)) and n_slots[g] == ns == len(pivot) and left[g] == lo == 0
    n_ops[3] = ops.shape[1] + 1; n_ops[4] = -1               # out of range: the pairs take no part
    mass2, _, _ = R.slot_mass(ops, n_ops, weight, pg, "ref", 80)
    assert not np.array_equal(mass2[0], mass[0]) and np.array_equal(mass2[1:], mass[1:])


def test_hyp_correct_statement():
    assert R.hyp_correct("abc", "xabcc") == [0.0, 1.0, 1.0, 0.0, 1.0]
    assert R.hyp_correct("abc", "") == [] and R.hyp_correct("", "ab") == [0.0, 0.0]
    assert R.hyp_correct("abc", "abd") == [1.0, 1.0, 0.0]


def test_predict_refuses_word_confidence_up_front(tmp_path):
    """Before anything is loaded: no list, a subword model, an unknown pivot, an alphabet without ' ' and one of more than 64
    symbols."""
    import os
    from policy_gradient_asr_amd import model
    with pytest.raises(ValueError, match="nbest >= 2"):
        model.predict(None, None, os.devnull, os.devnull, 1, word_confidence=True)
    with pytest.raises(ValueError, match="subword"):
        model.predict(None, None, os.devnull, os.devnull, 1, word_confidence=True, nbest=2, units_path=os.devnull)
    with pytest.raises(ValueError, match="confidence_pivot"):
        model.predict(None, None, os.devnull, os.devnull, 1, word_confidence=True, nbest=2, confidence_pivot="best")
    narrow = tmp_path / "narrow.txt"; narrow.write_text("a\nb\nc\n")
    with pytest.raises(ValueError, match="' ' symbol"):
        model.predict(None, None, str(narrow), str(tmp_path), 1, word_confidence=True, nbest=2)
    wide = tmp_path / "wide.txt"; wide.write_text("".join("u%d\n" % i for i in range(99)) + " \n")
    with pytest.raises(ValueError, match="word_confidence: not over"):
        model.predict(None, None, str(wide), str(tmp_path), 1, word_confidence=True, nbest=2, wide_beam=True)


def _nce_numpy(conf, correct, eps=1e-12):
    c = np.clip(np.asarray(conf, dtype=np.float64), eps, 1 - eps)
    k = np.asarray(correct, dtype=bool)
    p = k.mean()
    h_max = -(k.sum() * np.log2(p) + (~k).sum() * np.log2(1 - p))
    h = -(np.log2(c[k]).sum() + np.log2(1 - c[~k]).sum())
    return (h_max - h) / h_max


def test_confidence_nce():
    from policy_gradient_asr_amd.metrics import confidence_nce
    rng = np.random.default_rng(3)
    correct = (rng.random(200) < 0.7).astype(np.float64)
    base = correct.mean()
    assert abs(confidence_nce(correct, correct) - 1.0) < 1e-9                         # perfect: H_conf = 200 * -log2(1 - 1e-12)
    assert abs(confidence_nce(np.full(200, base), correct)) < 1e-12                   # the base rate: nothing learnt
    anti = confidence_nce(1.0 - correct, correct)
    assert anti < -10 and abs(anti - _nce_numpy(1.0 - correct, correct)) < 1e-9 * abs(anti)
    conf = rng.random(200)
    assert abs(confidence_nce(conf, correct) - _nce_numpy(conf, correct)) < 1e-12
    assert abs(R.nce(conf, correct) - _nce_numpy(conf, correct)) < 1e-12
    informed = np.where(correct > 0.5, 0.9, 0.2)
    assert 0 < confidence_nce(informed, correct) < 1
    assert abs(confidence_nce(conf.astype(np.float32), correct) - _nce_numpy(conf.astype(np.float32), correct)) < 1e-12
    for labels in (np.ones(5), np.zeros(5), np.zeros(0)):
        assert math.isnan(confidence_nce(np.full(labels.shape, 0.5), labels))
    with pytest.raises(ValueError):
        confidence_nce(np.zeros(3), np.zeros(4))
