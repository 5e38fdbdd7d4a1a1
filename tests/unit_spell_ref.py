"""Helper of the unit-spelling tests (not collected): the plain-Python statement of "spell the units, then count" -- join the unit
strings, map the characters to ids, split words with str.split(" "), Levenshtein by the plain DP -- written from the strings, not
from ``units.UnitSpelling``'s tables; the fixed case set that the CPU and GPU files share; and the policy-gradient objective of
oracle/pg_ref.py with the reward handed in (``objective``), so that the fp64 reference can take the spelled distances."""
from types import SimpleNamespace

import numpy as np

from oracle import ctc_ref, decode_ref, pg_ref


# ---- the statement ----
def text(units, ids):
    """units[i] is the string of token id i + 1; id 0 and ids outside 1 .. len(units) add nothing."""
    return "".join(units[int(i) - 1] for i in ids if 1 <= int(i) <= len(units))


def char_ids(units, ids, alphabet):
    """The spelled row: 1 + the index in ``alphabet`` of every character of the text."""
    return [alphabet.index(ch) + 1 for ch in text(units, ids)]


def levenshtein(a, b):
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def distances(units, ref_ids, hyp_ids):
    """(unit distance, character distance, word distance, characters of the reference, words of the reference)."""
    r, h = text(units, ref_ids), text(units, hyp_ids)
    ru = [int(i) for i in ref_ids if 1 <= int(i) <= len(units)]
    hu = [int(i) for i in hyp_ids if 1 <= int(i) <= len(units)]
    return levenshtein(ru, hu), levenshtein(r, h), levenshtein(r.split(" "), h.split(" ")), len(r), len(r.split(" "))


def spell_rows(units, alphabet, tokens, lengths, out_stride):
    """pgasr_unit_spell's contract on numpy rows: (out (N,out_stride), out_len (N,), full_len (N,)), zero behind out_len."""
    tokens, lengths = np.asarray(tokens), np.asarray(lengths)
    N, stride = tokens.shape
    out = np.zeros((N, out_stride), dtype=np.int32)
    out_len, full_len = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for n in range(N):
        row = char_ids(units, tokens[n, :min(max(int(lengths[n]), 0), stride)], alphabet)
        full_len[n] = len(row)
        out_len[n] = min(len(row), out_stride)
        out[n, :out_len[n]] = row[:out_stride]
    return out, out_len, full_len


# ---- the fixed cases: a small inventory whose units hold interior, leading and trailing spaces, and " " alone ----
ALPHABET = [" ", "a", "b", "c", "d", "e"]
UNITS = [" ", "a", "b", "c", "d", "e", "ab", "b c", " d", "e ", "cd", "a b", "de", "  "]
U = {u: i + 1 for i, u in enumerate(UNITS)}


def ids(*us):
    return [U[u] for u in us]


# (reference, hypothesis A, hypothesis B) in unit ids
CASES = {
    # A re-segments the reference (same text, same words, other units); B gets one character wrong inside one unit
    "resegmented": (ids("ab", " ", "cd", " ", "e"), ids("a", "b c", "d", " ", "e"), ids("ab", " ", "cd", " ", "d")),
    # one wrong unit of A breaks two words ("b c" -> "b"); B has three wrong units inside one word
    "unit-spans-space": (ids("a", "b c", "d"), ids("a", "b", "d"), ids("e", "b c", "cd", "de", "d")),
    # consecutive spaces: empty words count
    "empty-words": (ids("a", "  ", "b"), ids("a", " ", "b"), ids("a", " ", " ", "b")),
    # leading and trailing spaces
    "edges": (ids(" d", "e "), ids("d", "e"), ids(" ", "de", " ")),
    # A has one wrong character in each of two words, B three in one word: characters prefer A, words prefer B
    "char-vs-word": (ids("a", " ", "b", " ", "cd"), ids("e", " ", "e", " ", "cd"), ids("a", " ", "b", " ", "e", "e", "e")),
    "empty": ([], ids("a"), []),
}


def case_table():
    """name -> ((unit, char, word) distances of A, the same of B, C(y), W(y))."""
    out = {}
    for name, (ref, a, b) in CASES.items():
        da, db = distances(UNITS, ref, a), distances(UNITS, ref, b)
        out[name] = (da[:3], db[:3], da[3], da[4])
    return out


def random_units(V, seed, alphabet=None, max_chars=7, cap_unit=None):
    """V - 1 distinct units over ``alphabet`` (default: " " and 26 letters): the single characters first, then random strings of 2 ..
    max_chars characters with spaces anywhere; cap_unit: the length of one extra-long last unit."""
    alphabet = alphabet or [" "] + [chr(97 + i) for i in range(26)]
    rng = np.random.RandomState(seed)
    units, have = [], set()
    for ch in alphabet[:V - 1]:
        units.append(ch); have.add(ch)
    while len(units) < V - 1:
        n = int(rng.randint(2, max_chars + 1))
        if cap_unit and len(units) == V - 2:
            n = cap_unit
        u = "".join(alphabet[int(i)] for i in rng.randint(0, len(alphabet), size=n))
        if u not in have:
            units.append(u); have.add(u)
    return units, alphabet


# ---- the objective with the reward handed in ----
def objective(logits, in_len, targets, tg_len, reward, *, paths, greedy_frames, lam=1.0, baseline="hypothesis",
              score_function="path", max_hyp_len=None, entropy_weight=0.0, blank=0):
    """oracle.pg_ref.pg_objective on given frame paths (K,T,B) with R = reward(y, hyp): the CTC term, the K score terms
    (pg_ref.score_terms) and the entropy term (pg_ref.entropy_*) are the oracle's own; only the reward is the caller's.  With
    reward = -ED(units) / max(L,1) it is pg_objective itself (tests/test_unit_spell_cpu.py holds that)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    paths = np.asarray(paths, dtype=np.int64)
    K = paths.shape[0]
    in_len, tg_len = np.asarray(in_len), np.asarray(tg_len)
    lp = ctc_ref.log_softmax(logits, axis=2)
    ys = [[int(t) for t in targets[b][:tg_len[b]]] for b in range(B)]
    hyp = lambda frames, b: [int(t) for t in decode_ref.collapse_path(frames[:in_len[b], b], blank)]
    R = np.array([[reward(ys[b], hyp(paths[k], b)) for b in range(B)] for k in range(K)], dtype=np.float64)
    R_hyp = None
    if baseline == "hypothesis":
        R_hyp = np.array([reward(ys[b], hyp(np.asarray(greedy_frames), b)) for b in range(B)], dtype=np.float64)
        bk = np.broadcast_to(R_hyp, R.shape)
    else:
        bk = (R.sum(axis=0, keepdims=True) - R) / (K - 1)
    coef = lam * (R - bk) / (B * K)
    Lf = np.maximum(tg_len, 1).astype(np.float64)
    nll, g_ctc = ctc_ref.ctc_loss_and_grad(logits, targets, in_len, tg_len, blank)
    scale = 1.0 / (Lf * B)
    loss = (np.where(np.isfinite(nll), nll, 0.0) * scale).sum()
    grad = g_ctc * scale[None, :, None]
    s_loss, s_grad, hyps, scored = pg_ref.score_terms(logits, in_len, paths, coef, score_function, max_hyp_len, blank)
    loss, grad = loss + s_loss, grad + s_grad
    ent_mean, ent_scale = pg_ref.entropy_stats(lp, in_len, entropy_weight, 1.0 / B)
    if entropy_weight:
        loss += pg_ref.entropy_loss(lp, in_len, entropy_weight, 1.0 / B)
        grad = grad + pg_ref.entropy_grad(lp, in_len, ent_scale)
    return SimpleNamespace(loss=loss, grad=grad, nll=nll, R=R, R_hyp=R_hyp, baselines=bk, coef=coef, hyps=hyps, scored=scored,
                           ent_mean=ent_mean)


def spelled_reward(units, unit):
    """R = -ED(chars) / max(C(y),1) ("char") or -WED / W(y) ("word") of two unit-id lists."""
    def reward(y, hyp):
        _, dc, dw, C, W = distances(units, y, hyp)
        return -dc / max(C, 1) if unit == "char" else -dw / W
    return reward
