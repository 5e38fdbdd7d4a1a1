"""Helper of the single-wave LM-fusion tests (not collected): the cases of tests/test_beam_lm_fast_cpu.py and
tests/test_beam_lm_fast_gpu.py that tests/beam_lm_ref.py does not already hold -- the order-5 case at the table-size limit and the
MWER case with its language model -- and the limit table of pgasr_beam_lm_single_wave_ok."""
import functools

import numpy as np

import beam_lm_ref as R
import nbest_ref as NR

# The shared fp32 cases inside the single-wave kernel's limits (beam <= 16), and the one outside them (beam 100).
INSIDE = [c for c in R.FAST_CASES if c[2] <= 16]
OUTSIDE = [c for c in R.FAST_CASES if c[2] > 16]

# Order 5 at V = 29: 29^5 = 20 511 149 entries, just under the cap of 2^25 -- the context index arithmetic at its largest.
# (T, V, beam, order, blank, alpha, beta, seed); the seed was picked so that every utterance's margin is >= beam_lm_ref.GAP_MIN
# (test_beam_lm_fast_cpu.py asserts it).
ORDER5_CASE = (40, 29, 16, 5, 0, 0.6, 0.7, 0)


@functools.lru_cache(maxsize=None)
def order5_inputs():
    return R.fast_case_inputs(ORDER5_CASE)


@functools.lru_cache(maxsize=None)
def order5_reference():
    """Per utterance (prefix, score, gap) of the fused helper search; an utterance without frames: ((), -0.0, inf)."""
    T, V, beam, order, blank, alpha, beta, seed = ORDER5_CASE
    lp, lens, table = order5_inputs()
    out = []
    for b in range(R.FAST_B):
        n = int(lens[b])
        if n == 0:
            out.append(((), -0.0, float("inf")))
        else:
            out.append(R.fused_prefix_beam_search(logp=lp[:n, b].astype(np.float64), table=table, order=order, alpha=alpha, beta=beta,
                                                  beam_size=beam, blank=blank))
    return tuple(out)


# (T, V, beam, is_f64, lm_order) -> what pgasr_beam_lm_single_wave_ok answers: every limit just inside and just outside.
PREDICATE_TABLE = [
    ((1000, 29, 16, 0, 3), 1),
    ((1000, 29, 17, 0, 3), 0),                # beam 16 / 17
    ((300, 64, 16, 0, 2), 1),
    ((300, 65, 16, 0, 2), 0),                 # V 64 / 65
    ((1536, 29, 16, 0, 3), 1),                # T * beam = 24576
    ((24576, 29, 1, 0, 3), 0),                # ... the same product with T over 4096
    ((24577, 29, 1, 0, 3), 0),
    ((3511, 29, 7, 0, 3), 0),                 # T * beam = 24577 with T <= 4096
    ((8192, 29, 3, 0, 3), 0),                 # T * beam = 24576 but T > 4096
    ((4096, 29, 6, 0, 3), 1),                 # T 4096 (T * beam = 24576) / 4097
    ((4097, 29, 5, 0, 3), 0),
    ((4096, 29, 5, 0, 3), 1),
    ((1000, 29, 16, 1, 3), 0),                # fp64 log-probs
    ((1000, 29, 16, 0, 0), 0),                # no table
    ((1000, 29, 16, 0, -1), 0),
    ((1000, 29, 16, 0, 5), 1),                # 29^5 < 2^25
    ((1000, 29, 16, 0, 6), 0),                # a table the search refuses
    ((1, 4, 1, 0, 1), 1),
    ((0, 29, 16, 0, 3), 0), ((10, 0, 16, 0, 3), 0), ((10, 29, 0, 0, 3), 0),
]

# ---- MWER with a language model: the shape (T, B, V, beam, N, blank) = (40, 4, 6, 8, 4, 0) of test_mwer_gpu.LOSS_CASES ----
MWER_SHAPE = (40, 4, 6, 8, 4, 0)
MWER_SEED = 246
MWER_LM = (2, 2.0, 0.5, 9)                   # order, alpha, beta, table seed: alpha picked on the CPU so that the fused list differs


def mwer_case():
    """test_mwer_gpu._loss_case's recipe: (logits (T,B,V) fp32, targets (B,L) int32, in_len (B), tg_len (B)) as torch CPU tensors."""
    import torch
    T, B, V, beam, N, blank = MWER_SHAPE
    g = torch.Generator().manual_seed(MWER_SEED)
    logits = (torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2.0).float()
    in_len = torch.tensor([T, T - T // 4, T // 2, 1], dtype=torch.int32)
    tg_len = torch.tensor([max(1, min(6, T // 3)), max(1, min(5, T // 4)), max(1, min(4, T // 5)), 1], dtype=torch.int32)
    syms = torch.tensor([s for s in range(V) if s != blank])
    targets = syms[torch.randint(0, V - 1, (B, int(tg_len.max())), generator=g)].to(torch.int32)
    for b in range(B):
        targets[b, int(tg_len[b]):] = 0
    return logits, targets, in_len, tg_len


def mwer_table():
    T, B, V, beam, N, blank = MWER_SHAPE
    return R.random_table(V, MWER_LM[0], blank, MWER_LM[3])


def mwer_lists(with_lm):
    """The helper's N-best lists of the MWER case per utterance, [(prefix, score)], gap: the acoustic search or the fused one."""
    T, B, V, beam, N, blank = MWER_SHAPE
    logits, _, in_len, _ = mwer_case()
    lp = R.log_softmax32(logits.double().numpy())
    order, alpha, beta, _ = MWER_LM
    out = []
    for b in range(B):
        n = int(in_len[b])
        out.append(NR.nbest_prefix_beam_search(logp=lp[:n, b].astype(np.float64), table=mwer_table() if with_lm else None,
                                               order=order if with_lm else 0, alpha=alpha if with_lm else 0.0,
                                               beta=beta if with_lm else 0.0, beam_size=beam, blank=blank, nbest=N))
    return out
