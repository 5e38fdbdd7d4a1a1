"""Plain Python statement of the N-best confidence (include/pgasr_hip.h, A10-CONF; csrc/confidence.hip), built on
tests/editops_ref.py's canonical alignment.  Loops over pairs and operations, Python floats added in the stated order: what the
kernel has to reproduce bit for bit."""
import math

import numpy as np

import editops_ref

HIT, SUB, DEL, INS = editops_ref.HIT, editops_ref.SUB, editops_ref.DEL, editops_ref.INS
SIDES = {"ref": 0, "hyp": 1}


def _side(side):
    side = SIDES.get(side, side)
    if side not in (0, 1):
        raise ValueError("side must be 'ref' / 0 or 'hyp' / 1")
    return side


def slot_count(ops, side):
    """The number of slot-consuming operations of one operation list."""
    other = INS if _side(side) == 0 else DEL
    return sum(1 for o in ops if 0 <= o <= 3 and o != other)


def participates(w, n_ops, ops_stride):
    return math.isfinite(w) and w > 0 and 0 <= n_ops <= ops_stride


def group_mass(op_lists, weights, side, slots, ops_stride=None):
    """One group: op_lists a list of operation lists (or None for a pair whose n_ops is out of range), weights as many floats.
    Returns (mass [4][slots + 1] of Python floats, n_slots, left_out)."""
    side = _side(side)
    own, other = (DEL, INS) if side == 0 else (INS, DEL)
    mass = [[0.0] * (slots + 1) for _ in range(4)]
    n_slots, left_out = -1, 0
    for ops, w in zip(op_lists, weights):
        w = float(w)
        if ops is None or not participates(w, len(ops), len(ops) if ops_stride is None else ops_stride):
            continue
        c = slot_count(ops, side)
        if n_slots < 0:
            n_slots = c
        if c != n_slots or c > slots:
            left_out += 1
            continue
        slot = 0
        k = [0] * (n_slots + 1)
        for o in ops:
            if o == other:
                k[slot] += 1
            elif 0 <= o <= 3:
                ch = 2 if o == own else o
                mass[ch][slot] = mass[ch][slot] + w
                slot += 1
        for j in range(n_slots + 1):
            if k[j] > 0:
                mass[3][j] = mass[3][j] + w * float(k[j])
    return mass, n_slots, left_out


def slot_mass(ops, n_ops, weight, per_group, side, slots):
    """The launch: ops (P, ops_stride) int8 / n_ops (P) / weight (P) as numpy arrays, P = groups * per_group.  Returns
    (mass (groups, 4, slots + 1) float64, n_slots (groups) int32, left_out (groups) int32)."""
    ops, n_ops, weight = np.asarray(ops), np.asarray(n_ops), np.asarray(weight, dtype=np.float64)
    P, stride = ops.shape
    assert P % per_group == 0
    groups = P // per_group
    mass = np.zeros((groups, 4, slots + 1), dtype=np.float64)
    ns = np.zeros(groups, dtype=np.int32)
    lo = np.zeros(groups, dtype=np.int32)
    for g in range(groups):
        lists = []
        for p in range(g * per_group, (g + 1) * per_group):
            k = int(n_ops[p])
            lists.append([int(x) for x in ops[p, :k]] if 0 <= k <= stride else None)
        m, ns[g], lo[g] = group_mass(lists, [float(x) for x in weight[g * per_group:(g + 1) * per_group]], side, slots, stride)
        mass[g] = np.asarray(m, dtype=np.float64)
    return mass, ns, lo


def nbest_confidence(rows, posterior, pivot, slots=None):
    """One utterance: rows a list of symbol sequences (characters, words, ids), posterior as many floats, pivot an index.
    Every row is aligned to the pivot row (the pivot is the REFERENCE of tests/editops_ref.py's alignment); returns
    (conf, substituted, deleted, inserted, left_out), the first four lists of len(pivot row) + 1 floats -- the last cell is 0
    except inserted's, the gap behind the last position -- or of slots + 1 when slots is given."""
    piv = list(rows[pivot])
    # the pivot's own pair stands where it stands in the list: ascending n is the order of the additions.  Every pair has the pivot
    # as its reference, so every slot count is len(piv)
    lists = [editops_ref.edit_ops(piv, list(rows[n]))[1] for n in range(len(rows))]
    L = len(piv) if slots is None else slots
    mass, n_slots, left_out = group_mass(lists, posterior, "ref", L)
    return mass[0], mass[1], mass[2], mass[3], left_out


def words_of(row, delimiter):
    """str.split(" ") on a token row: n delimiters give n + 1 words (tuples of tokens), empty ones included."""
    words, cur = [], []
    for t in row:
        if t == delimiter:
            words.append(tuple(cur)); cur = []
        else:
            cur.append(t)
    words.append(tuple(cur))
    return words


def hyp_correct(ref, hyp):
    """Per hypothesis position 1.0 where the canonical alignment to the reference has a hit there."""
    ops = editops_ref.edit_ops(list(ref), list(hyp))[1]
    return [1.0 if o == HIT else 0.0 for o in ops if o != DEL]


def nce(conf, correct, eps=1e-12):
    """NIST's normalised cross entropy in bits, evaluated directly; NaN when all or none are correct."""
    conf = np.clip(np.asarray(conf, dtype=np.float64), eps, 1.0 - eps)
    correct = np.asarray(correct, dtype=np.float64) > 0.5
    n, nc = correct.size, int(correct.sum())
    if n == 0 or nc == 0 or nc == n:
        return float("nan")
    pc = nc / n
    h_max = -(nc * math.log2(pc) + (n - nc) * math.log2(1.0 - pc))
    h_conf = -(np.log2(conf[correct]).sum() + np.log2(1.0 - conf[~correct]).sum())
    return float((h_max - h_conf) / h_max)
