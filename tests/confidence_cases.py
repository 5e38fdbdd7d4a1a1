"""The inputs of the slot-mass tests, shared by tests/test_confidence_cpu.py (which proves them discriminating: ties in most random
pairs, several insertions in one gap in every case) and tests/test_confidence_gpu.py (which holds csrc/confidence.hip to
tests/confidence_ref.py on them).  Everything is seed-fixed; operation strings come from tests/editops_ref.py, which
tests/test_editops_gpu.py holds the device's alignment to bit for bit."""
import functools

import numpy as np

import editops_ref

FOREIGN = 99                     # a symbol no generated row holds: inserted into a copy of the pivot it leaves ONE optimal alignment
CHUNK = 512                      # csrc/confidence.hip: operations per pass of the workgroup

# target operation-string lengths: the issue's list, and this kernel's own seams at multiples of 512
OP_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 1860)
# (per_group, groups)
GROUP_SHAPES = tuple((pg, g) for pg in (1, 2, 16, 128) for g in (1, 5))


def hand_case():
    """The hand-worked list: pivot "abc"; every mass is a short binary fraction."""
    rows = ["abc", "abd", "ac", "xabcc"]
    weights = [0.5, 0.25, 0.125, 0.125]
    want = {"conf": [1.0, 0.875, 0.75, 0.0], "substituted": [0.0, 0.0, 0.25, 0.0], "deleted": [0.0, 0.125, 0.0, 0.0],
            "inserted": [0.125, 0.0, 0.125, 0.0]}
    return rows, weights, want


def _insert_run(pivot, k, at):
    return pivot[:at] + [FOREIGN] * k + pivot[at:]


def _group(rng, n, per_group, vocab=4, exact_extra=3):
    """One group around a random pivot of n symbols: (pivot, rows, random_flags).  Row 0 is the pivot itself (n operations), row 1
    the pivot with ``exact_extra`` foreign symbols in one gap (exactly n + exact_extra operations, several insertions in one gap),
    the others edited copies of about the same length (random_flags marks them)."""
    pivot = rng.integers(0, vocab, n).tolist()
    rows, random_flags = [], []
    for r in range(per_group):
        if r == 0:
            rows.append(list(pivot)); random_flags.append(False)
        elif r == 1:
            rows.append(_insert_run(pivot, exact_extra, int(rng.integers(0, n + 1)))); random_flags.append(False)
        else:
            rows.append(_mutate(rng, list(pivot), max(0, n + int(rng.integers(-3, 4))), vocab)); random_flags.append(True)
    return pivot, rows, random_flags


def _mutate(rng, ref, m, vocab):
    """An edited copy of ref with m symbols (deletions, substitutions, insertions, double insertions)."""
    hyp = []
    for s in ref:
        u = rng.random()
        if u < 0.1:
            continue
        hyp.append(int(rng.integers(0, vocab)) if u < 0.25 else s)
        if u > 0.9:
            hyp += [int(rng.integers(0, vocab)) for _ in range(2)]
    while len(hyp) < m:
        hyp.insert(int(rng.integers(0, len(hyp) + 1)), int(rng.integers(0, vocab)))
    while len(hyp) > m:
        del hyp[int(rng.integers(0, len(hyp)))]
    return hyp


def _weights(rng, n):
    w = rng.random(n) + 1e-3
    return (w / w.sum()).tolist()


@functools.lru_cache(maxsize=None)
def length_cases():
    """One group per target length K: [(K, pivot, rows, weights, random_flags)], four rows each (two for the empty pivot's K = 0:
    the pivot's own pair then HAS 0 operations).  For K >= 3 row 1 has exactly K operations; the pivot's own pair has K - 3; K = 1
    is a pivot of one symbol."""
    rng = np.random.default_rng(20240901)
    out = []
    for K in OP_LENGTHS:
        n = K - 3 if K >= 3 else K
        pivot, rows, flags = _group(rng, n, 4)
        out.append((K, pivot, rows, _weights(rng, len(rows)), flags))
    return out


@functools.lru_cache(maxsize=None)
def shape_cases():
    """[(per_group, groups, [(pivot, rows, weights, random_flags)] per group)] with pivots of 5 .. 70 symbols."""
    rng = np.random.default_rng(20240902)
    out = []
    for pg, G in GROUP_SHAPES:
        groups = []
        for g in range(G):
            n = int(rng.integers(5, 71))
            pivot, rows, flags = _group(rng, n, max(pg, 2))
            if pg == 1:                                  # the one pair: the row with the run of insertions
                rows, flags = rows[1:2], flags[1:2]
            groups.append((pivot, rows, _weights(rng, pg), flags))
        out.append((pg, G, groups))
    return out


def op_lists(pivot, rows, side):
    """The operation lists of a group: side "ref" aligns (pivot, row), side "hyp" (row, pivot) -- the pivot's positions are the
    slots either way."""
    return [list(o) for o in _op_lists(tuple(pivot), tuple(tuple(r) for r in rows), side)]


@functools.lru_cache(maxsize=None)
def _op_lists(pivot, rows, side):
    pivot = list(pivot)
    if side == "ref":
        return tuple(tuple(editops_ref.edit_ops(pivot, list(r))[1]) for r in rows)
    return tuple(tuple(editops_ref.edit_ops(list(r), pivot)[1]) for r in rows)


def mirror(ops):
    """The same alignment seen from the swapped pair: deletions and insertions change places."""
    return [{2: 3, 3: 2}.get(o, o) for o in ops]


def has_run_of_other(ops, side, k=2):
    """True iff some gap of the list holds k or more "other" operations (insertions for side "ref")."""
    other = 3 if side == "ref" else 2
    run = 0
    for o in ops:
        run = run + 1 if o == other else 0
        if run >= k:
            return True
    return False


def pack_ops(lists, stride=None, extra=5, fill=-1):
    """Operation lists -> (ops (P, stride) int8 with ``fill`` behind every list, n_ops (P) int32)."""
    longest = max((len(o) for o in lists), default=0)
    stride = longest + extra if stride is None else stride
    ops = np.full((len(lists), stride), fill, dtype=np.int8)
    n_ops = np.zeros(len(lists), dtype=np.int32)
    for p, o in enumerate(lists):
        ops[p, :len(o)] = o
        n_ops[p] = len(o)
    return ops, n_ops
