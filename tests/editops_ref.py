"""Plain Python / numpy reference of the edit-operation alignment (include/pgasr_hip.h, A10-OPS; csrc/editops.hip).

D[i][j] is the Levenshtein matrix over reference prefix i and hypothesis prefix j (sub = ins = del = 1).  The canonical alignment
walks back from (n, m): the diagonal if it is optimal, else the deletion (a reference symbol without partner) if it is optimal, else
the insertion.  Operations: 0 = hit, 1 = substitution, 2 = deletion, 3 = insertion, left to right."""
import numpy as np

HIT, SUB, DEL, INS = 0, 1, 2, 3
CANONICAL = ("diag", "del", "ins")


def matrix(ref, hyp):
    """The full matrix, a numpy row at a time: x[j] = min(up + 1, diagonal + mismatch), then the chain of insertions along the row
    as a running minimum of x[j] - j.  ``matrix_naive`` is the cell-by-cell definition it is tested against."""
    n, m = len(ref), len(hyp)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    idx = np.arange(m + 1, dtype=np.int32)
    D[0] = idx
    table = {}                                   # any hashable symbols (characters, words, ids)
    r = [table.setdefault(s, len(table)) for s in ref]
    h = np.asarray([table.setdefault(s, len(table)) for s in hyp], dtype=np.int64)
    for i in range(1, n + 1):
        x = np.empty(m + 1, dtype=np.int32)
        x[0] = i
        if m:
            x[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (h != r[i - 1]))
        D[i] = np.minimum.accumulate(x - idx) + idx
    return D


def matrix_naive(ref, hyp):
    n, m = len(ref), len(hyp)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[:, 0] = np.arange(n + 1)
    D[0, :] = np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    return D


def walk(ref, hyp, D=None, order=CANONICAL):
    """The operation string of the alignment that takes, at every cell, the first optimal move in ``order``."""
    if D is None:
        D = matrix(ref, hyp)
    i, j = len(ref), len(hyp)
    ops = []
    while i > 0 or j > 0:
        for move in order:
            if move == "diag" and i > 0 and j > 0 and D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]) == D[i, j]:
                ops.append(SUB if ref[i - 1] != hyp[j - 1] else HIT); i -= 1; j -= 1
                break
            if move == "del" and i > 0 and D[i - 1, j] + 1 == D[i, j]:
                ops.append(DEL); i -= 1
                break
            if move == "ins" and j > 0 and D[i, j - 1] + 1 == D[i, j]:
                ops.append(INS); j -= 1
                break
        else:
            raise AssertionError("no optimal move: D is not a Levenshtein matrix")
    return ops[::-1]


def counts_of(ops):
    return [sum(1 for o in ops if o == k) for k in (HIT, SUB, DEL, INS)]


def edit_ops(ref, hyp, order=CANONICAL):
    """(counts [H, S, D, I], ops) of one pair."""
    ops = walk(ref, hyp, order=order)
    return counts_of(ops), ops


def confusion_add(cm, ref, hyp, ops, vocab):
    """Add one pair's operations into cm ((vocab+1, vocab+1) int64): [r][h] hits and substitutions, [r][vocab] deletions,
    [vocab][h] insertions; an operation with a symbol outside [0, vocab) is left out."""
    i = j = 0
    ok = lambda s: 0 <= s < vocab
    for o in ops:
        if o in (HIT, SUB):
            if ok(ref[i]) and ok(hyp[j]):
                cm[ref[i], hyp[j]] += 1
            i += 1; j += 1
        elif o == DEL:
            if ok(ref[i]):
                cm[ref[i], vocab] += 1
            i += 1
        else:
            if ok(hyp[j]):
                cm[vocab, hyp[j]] += 1
            j += 1
    assert i == len(ref) and j == len(hyp)
    return cm


def count_optimal_alignments(ref, hyp, D=None):
    """How many optimal alignments (paths of optimal moves from (n, m) to (0, 0)) the pair has."""
    if D is None:
        D = matrix(ref, hyp)
    n, m = len(ref), len(hyp)
    P = [[0] * (m + 1) for _ in range(n + 1)]
    P[0][0] = 1
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            c = 0
            if i > 0 and j > 0 and D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]) == D[i, j]:
                c += P[i - 1][j - 1]
            if i > 0 and D[i - 1, j] + 1 == D[i, j]:
                c += P[i - 1][j]
            if j > 0 and D[i, j - 1] + 1 == D[i, j]:
                c += P[i][j - 1]
            P[i][j] = c
    return P[n][m]


def all_alignments(ref, hyp):
    """Every monotone alignment of the pair (optimal or not) as an operation list, in the lexicographic order of a walk BACK from
    (n, m) that tries diagonal, deletion, insertion -- exhaustive enumeration for tiny strings."""
    out = []

    def rec(i, j, ops):
        if i == 0 and j == 0:
            out.append(ops[::-1])
            return
        if i > 0 and j > 0:
            rec(i - 1, j - 1, ops + [SUB if ref[i - 1] != hyp[j - 1] else HIT])
        if i > 0:
            rec(i - 1, j, ops + [DEL])
        if j > 0:
            rec(i, j - 1, ops + [INS])
    rec(len(ref), len(hyp), [])
    return out


def cost(ops):
    return sum(1 for o in ops if o != HIT)


def clamp_rows(rows, lens, stride):
    """The rows as the kernel sees them: lengths clamped to [0, stride]."""
    return [list(map(int, rows[k][:min(max(int(lens[k]), 0), stride)])) for k in range(len(lens))]


def batch(ref, ref_len, hyp, hyp_len, vocab=None):
    """numpy (N,R) / (N,Hy) rows with lengths -> counts (N,4) int32, ops (N,R+Hy) int8 with -1 tail, n_ops (N) int32, and the
    confusion matrix (vocab given) or None."""
    ref, hyp = np.asarray(ref), np.asarray(hyp)
    N, R, Hy = ref.shape[0], ref.shape[1], hyp.shape[1]
    rr, hh = clamp_rows(ref, ref_len, R), clamp_rows(hyp, hyp_len, Hy)
    counts = np.zeros((N, 4), dtype=np.int32)
    ops = np.full((N, R + Hy), -1, dtype=np.int8)
    n_ops = np.zeros(N, dtype=np.int32)
    cm = None if vocab is None else np.zeros((vocab + 1, vocab + 1), dtype=np.int64)
    for k in range(N):
        c, o = edit_ops(rr[k], hh[k])
        counts[k] = c; ops[k, :len(o)] = o; n_ops[k] = len(o)
        if cm is not None:
            confusion_add(cm, rr[k], hh[k], o, vocab)
    return counts, ops, n_ops, cm
