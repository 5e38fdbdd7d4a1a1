"""Planted CTC inputs shared by tests/test_ctc_cases_cpu.py and tests/test_ctc_numerics_gpu.py (TEST INFRASTRUCTURE ONLY).

A random-logit case is flat: every row's maximum sits near -ln V and nothing is ever far from anything else.  ``planted`` builds
the other regime on purpose: one valid alignment per utterance gets ``scale`` added to its symbol's logit at every frame, so the
rows are peaked like a trained model's (``sat*``), or the peak is put on the WRONG symbol (``anti*``), so that the target stays
feasible but every frame of every alignment costs about ``scale`` nats and the row maxima of alpha and beta fall by that much
per frame.  CASES is the table of NOTES.md 0.14: the smallest shapes at which each mechanism of csrc/ctc.hip is still exercised.
"""
import functools

import numpy as np
import torch

from oracle import ctc_ref


def planted(T, B, V, L, seed, scale, blank=0, il=None, tl=None, repeats=False, anti=False, pad_garbage=False):
    """-> logits (T,B,V) fp32, targets (B,max(L,1)) int32, il (B,) int32, tl (B,) int32.

    N(0,1) logits; targets drawn from the non-blank symbols (with blank != 0, symbol 0 is every utterance's first label);
    ``repeats`` makes every odd target position equal the one before it (the skip rule); one alignment per utterance -- a blank
    between equal neighbours, the spare frames spread at random as blanks -- gets ``scale`` added to its symbol's logit at every
    frame, or with ``anti`` to (symbol + 1) % V; ``pad_garbage`` fills the target columns at and beyond tl[b] with -1 and V + 5."""
    rng = np.random.default_rng(seed)
    il = np.full(B, T, np.int32) if il is None else np.asarray(il, np.int32)
    tl = np.full(B, L, np.int32) if tl is None else np.asarray(tl, np.int32)
    assert il.shape == tl.shape == (B,) and il.max() <= T and tl.max() <= L
    logits = rng.normal(size=(T, B, V))
    symbols = np.array([v for v in range(V) if v != blank])
    targets = rng.choice(symbols, size=(B, max(L, 1))).astype(np.int32)
    if blank != 0:
        targets[:, 0] = 0
    if repeats:
        for i in range(1, L, 2):
            targets[:, i] = targets[:, i - 1]
    for b in range(B):
        Tb, Lb = int(il[b]), int(tl[b])
        seq = []                       # the shortest frame labelling that collapses to the target
        for i in range(Lb):
            if i and targets[b, i] == targets[b, i - 1]:
                seq.append(blank)
            seq.append(int(targets[b, i]))
        spare = Tb - len(seq)
        if spare < 0:
            raise ValueError(f"utterance {b}: {Tb} frames cannot align {Lb} labels")
        gaps = rng.multinomial(spare, np.full(len(seq) + 1, 1.0 / (len(seq) + 1)))
        frames = [blank] * gaps[0]
        for i, v in enumerate(seq):
            frames += [v] + [blank] * gaps[i + 1]
        frames = np.asarray(frames, dtype=np.int64)
        assert frames.size == Tb
        if anti:
            frames = (frames + 1) % V
        logits[np.arange(Tb), b, frames] += scale
    if pad_garbage:
        for b in range(B):
            pad = targets[b, int(tl[b]):]
            pad[0::2] = -1
            pad[1::2] = V + 5
    return logits.astype(np.float32), targets, il, tl


# name -> planted()'s arguments (NOTES.md 0.14 says what each one is there for)
CASES = {
    "sat8": dict(T=64, B=4, V=29, L=10, scale=8.0, il=[64, 63, 62, 61], tl=[10, 9, 7, 4]),   # one il per T mod 4; ragged tl
    "sat20": dict(T=64, B=4, V=29, L=10, scale=20.0),
    "sat40": dict(T=300, B=3, V=29, L=60, scale=40.0),
    "anti20": dict(T=120, B=3, V=29, L=20, scale=20.0, anti=True),
    "anti40": dict(T=120, B=3, V=29, L=20, scale=40.0, anti=True),      # a row reference stale by up to 3 frames of -40 each
    "rep": dict(T=90, B=3, V=5, L=30, scale=10.0, repeats=True),
    "blank_last": dict(T=80, B=3, V=64, L=12, scale=12.0, blank=63, tl=[12, 9, 5], pad_garbage=True),
    "blank_mid": dict(T=50, B=3, V=29, L=8, scale=6.0, blank=3),
    "min_T": dict(T=41, B=2, V=29, L=20, scale=6.0),                    # T = 2L + 1
    "S63": dict(T=140, B=2, V=29, L=31, scale=10.0),                    # 64-state groups of the storer: S = 63 / 65
    "S65": dict(T=140, B=2, V=29, L=32, scale=10.0),
    "S255": dict(T=300, B=2, V=29, L=127, scale=10.0),                  # one / two states per thread: S = 255 / 257
    "S257": dict(T=300, B=2, V=29, L=128, scale=10.0),
    "nspt4": dict(T=640, B=2, V=29, L=300, scale=10.0, il=[640, 601], tl=[300, 256]),        # utterance 1: S = 513
    "nspt8": dict(T=1230, B=2, V=29, L=600, scale=10.0, il=[1230, 1101], tl=[600, 512]),     # utterance 1: S = 1025
    "tiny_L0": dict(T=1, B=1, V=2, L=0, scale=3.0),
    "tiny_T1": dict(T=1, B=1, V=2, L=1, scale=3.0),
    "tiny_T2": dict(T=2, B=1, V=3, L=1, scale=3.0),
    "tiny_empty": dict(T=3, B=2, V=4, L=1, scale=3.0, il=[3, 0], tl=[1, 0]),                 # an utterance without frames
}
ANTI = tuple(n for n, kw in CASES.items() if kw.get("anti"))
SEED = 1


def torch_ctc(logits, targets, il, tl, blank, dtype):
    """torch's CPU ctc_loss plus autograd through log_softmax in ``dtype``: (nll (B,), d sum(nll) / d logits (T,B,V)) as fp64."""
    x = torch.tensor(np.asarray(logits), dtype=dtype, requires_grad=True)
    nll = torch.nn.functional.ctc_loss(torch.log_softmax(x, 2), torch.tensor(np.asarray(targets)).long().clamp(min=0),
                                       torch.tensor(np.asarray(il)).long(), torch.tensor(np.asarray(tl)).long(),
                                       blank=blank, reduction="none", zero_infinity=False)
    nll.sum().backward()
    return nll.detach().double().numpy(), x.grad.double().numpy()


class Case:
    """One row of CASES with its references, computed once and read-only: the fp64 oracle on the fp32 logits (nll, grad) and the
    error of torch's fp32 CPU ctc_loss + autograd on the same input against it (e32_nll, e32_grad)."""

    def __init__(self, name):
        kw = CASES[name]
        self.name, self.blank, self.T = name, kw.get("blank", 0), kw["T"]
        self.logits, self.targets, self.il, self.tl = planted(seed=SEED, **kw)
        self.nll, self.grad = ctc_ref.ctc_loss_and_grad(self.logits, self.targets, self.il, self.tl, blank=self.blank)
        n32, g32 = torch_ctc(self.logits, self.targets, self.il, self.tl, self.blank, torch.float32)
        self.e32_nll = float(np.abs(n32 - self.nll).max())
        self.e32_grad = float(np.abs(g32 - self.grad).max())
        for a in (self.logits, self.targets, self.il, self.tl, self.nll, self.grad):
            a.setflags(write=False)

    def torch64(self):
        return torch_ctc(self.logits, self.targets, self.il, self.tl, self.blank, torch.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- exact zero probabilities ----
def _small(seed=3):
    return planted(T=30, B=2, V=8, L=4, seed=seed, scale=5.0)


def masked_case():
    """T = 30, B = 2, V = 8, L = 4, scale 5 with a logit of -inf (p = 0 exactly) at one frame each for the blank (utterance 0),
    a label of the target (utterance 0) and a symbol outside the target (utterance 1).  The masked frames are ones where the
    planted alignment emits another symbol, so every utterance stays alignable.  -> logits, targets, il, tl, masked [(t, b, v)]."""
    logits, targets, il, tl = _small()
    peak = logits.argmax(axis=2)                 # the planted frame labels (scale 5 against N(0,1) noise)
    label = int(targets[0, 1])
    outside = next(v for v in range(1, 8) if v not in targets[1])
    t_blank = next(t for t in range(5, 30) if peak[t, 0] != 0)
    t_label = next(t for t in range(7, 30) if peak[t, 0] not in (0, label) and t != t_blank)
    masked = [(t_blank, 0, 0), (t_label, 0, label), (9, 1, outside)]
    for t, b, v in masked:
        logits[t, b, v] = -np.inf
    return logits, targets, il, tl, masked


def impossible_label_case():
    """masked_case's shapes with one target label of utterance 0 at -inf on EVERY frame: no alignment exists for that utterance."""
    logits, targets, il, tl = _small()
    logits[:, 0, int(targets[0, 1])] = -np.inf
    return logits, targets, il, tl
