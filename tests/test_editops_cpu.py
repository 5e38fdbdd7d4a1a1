"""The statement of the edit-operation alignment (tests/editops_ref.py; include/pgasr_hip.h, A10-OPS) against exhaustive
enumeration and the project's oracles, the proof that the GPU test's inputs are discriminating, and the host-only workspace query
of csrc/editops.hip.  No GPU."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import editops_cases as C
import editops_ref as R
from oracle import decode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")


def test_canonical_alignment_against_exhaustive_enumeration():
    """Every pair of strings of length <= 4 over 2 symbols: among ALL alignments the cheapest cost is D[n][m], the canonical
    alignment has it, and it is the first cheapest one in the order diagonal, deletion, insertion of the walk back -- i.e. the one
    the rule picks."""
    strings = [list(s) for L in range(5) for s in itertools.product((0, 1), repeat=L)]
    assert len(strings) == 31
    for ref in strings:
        for hyp in strings:
            every = R.all_alignments(ref, hyp)
            best = min(R.cost(a) for a in every)
            D = R.matrix(ref, hyp)
            got = R.walk(ref, hyp, D)
            assert best == D[len(ref), len(hyp)] == R.cost(got)
            assert got == next(a for a in every if R.cost(a) == best), (ref, hyp)
            assert R.count_optimal_alignments(ref, hyp, D) == sum(1 for a in every if R.cost(a) == best)


def test_matrix_rows_against_the_cell_definition():
    rng = np.random.default_rng(3)
    for n, m, v in ((0, 0, 2), (0, 5, 2), (5, 0, 2), (1, 1, 2), (17, 23, 2), (40, 31, 4), (64, 65, 29)):
        ref, hyp = rng.integers(0, v, n).tolist(), rng.integers(0, v, m).tolist()
        assert np.array_equal(R.matrix(ref, hyp), R.matrix_naive(ref, hyp))
    assert np.array_equal(R.matrix("kitten", "sitting"), R.matrix_naive("kitten", "sitting"))


def test_identities_on_random_pairs():
    rng = np.random.default_rng(11)
    for _ in range(60):
        v = int(rng.choice((2, 4, 29)))
        n, m = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        ref, hyp = C._rows(rng, v, n, m, mutate=bool(rng.integers(0, 2)))
        (H, S, D, I), ops = R.edit_ops(ref, hyp)
        assert H + S + D == n and H + S + I == m and len(ops) == H + S + D + I
        assert S + D + I == R.matrix(ref, hyp)[n, m] == decode_ref.edit_dist(ref, hyp)[0]
        cm = R.confusion_add(np.zeros((v + 1, v + 1), dtype=np.int64), ref, hyp, ops, v)
        assert cm.sum() == len(ops) and np.trace(cm[:v, :v]) == H
        assert cm[:v, v].sum() == D and cm[v, :v].sum() == I and cm[v, v] == 0


def test_distance_agrees_with_the_golden_fixtures(golden_dir):
    vectors = json.load(open(os.path.join(golden_dir, "reference_vectors.json")))
    seen = 0
    for key in ("edit_dist", "edit_dist_tokens"):
        for a, b, want in vectors["text"][key]:
            (H, S, D, I), _ = R.edit_ops(a, b)
            assert [S + D + I, H + S + D] == want
            seen += 1
    assert seen >= 4


def test_the_gpu_cases_are_discriminating():
    """Every tie case has more than one optimal alignment, and under the order deletion > insertion > diagonal at least a third of
    them get other counts: a kernel with another tie rule cannot pass them."""
    cases = C.tie_cases()
    moved = 0
    for name, ref, hyp in cases:
        D = R.matrix(ref, hyp)
        assert R.count_optimal_alignments(ref, hyp, D) > 1, name
        moved += R.counts_of(R.walk(ref, hyp, D)) != R.counts_of(R.walk(ref, hyp, D, order=("del", "ins", "diag")))
    assert 3 * moved >= len(cases), (moved, len(cases))
    # a kernel that lays the longer sequence across its lanes and forgets that the rule follows the swap takes insertion before
    # deletion exactly where the hypothesis is the longer one: several such cases must give another string then
    swapped = [(r, h) for _, r, h in cases if len(h) > len(r)]
    assert sum(R.walk(r, h) != R.walk(r, h, order=("diag", "ins", "del")) for r, h in swapped) >= 4


def test_length_cases_cover_both_ways_round():
    for longer in C.TILING_LENGTHS[1:] + C.LONG_LENGTHS:
        pairs = C.length_pairs(longer)
        assert (longer, longer) in pairs and any(n > m for n, m in pairs) and any(m > n for n, m in pairs)
        assert (longer, 0) in pairs and (0, longer) in pairs
    assert C.length_pairs(0) == [(0, 0)]
    for n, m, ref, hyp in C.length_cases() + C.long_cases():
        assert len(ref) == n and len(hyp) == m


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.pgasr_edit_ops_workspace_bytes.restype = ctypes.c_size_t
    lib.pgasr_edit_ops_workspace_bytes.argtypes = [ctypes.c_int] * 3
    return lib


def test_workspace_query_needs_no_gpu(lib):
    q = lib.pgasr_edit_ops_workspace_bytes
    # a quarter byte per DP cell: one pair at the limit needs at least 4095 * 4096 / 4 bytes, and no more than twice that
    assert 4095 * 4096 // 4 <= q(4095, 4095, 1) <= 2 * 4096 * 4096 // 4
    assert q(4095, 4095, 7) == 7 * q(4095, 4095, 1)
    assert q(100, 100, 1) >= 100 * 101 // 4 and q(100, 100, 1) <= 8 * 1024
    assert q(4096, 10, 1) == 0 and q(10, 4096, 1) == 0 and q(10, 10, 0) == 0 and q(-1, 10, 1) == 0
    assert q(0, 50, 3) == 0 and q(50, 0, 3) == 0               # an empty side: nothing to walk back over
    sizes = (0, 1, 15, 16, 17, 62, 63, 64, 65, 126, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4094, 4095)
    for other in (1, 63, 64, 300, 4095):
        for lo, hi in zip(sizes, sizes[1:]):
            assert q(lo, other, 2) <= q(hi, other, 2), (lo, hi, other)
            assert q(other, lo, 2) <= q(other, hi, 2), (lo, hi, other)
    for n in range(1, 6):
        assert q(129, 70, n) < q(129, 70, n + 1)
    # enough for the 2-bit choices of every cell the walk can visit
    for rs, hs in ((1, 1), (63, 63), (64, 3), (3, 64), (100, 1000), (1000, 100), (4095, 1)):
        assert q(rs, hs, 1) * 4 >= min(rs, hs) * (max(rs, hs) + 1)


def test_python_wrapper_of_the_query():
    from policy_gradient_asr_amd import hipops
    assert hipops.edit_ops_workspace_bytes(4095, 4095, 1) >= 4095 * 4096 // 4
    assert hipops.edit_ops_workspace_bytes(100, 100, 32) == 32 * hipops.edit_ops_workspace_bytes(100, 100, 1)
