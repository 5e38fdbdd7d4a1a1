"""Helper of tests/test_wide_pg_cpu.py and tests/test_wide_pg_gpu.py (not collected): the sampler inputs of
tests/test_wide_vocab_gpu.py restated, their K = 16 draws by oracle.pg_ref.sample_paths (computed once, read-only), the project's
rule for a draw that differs from them, and a plain float32 restatement of the kernels' cdf rule in numpy."""
import functools

import numpy as np
import torch

from oracle import pg_ref

WIDE_V = [65, 128, 129, 257, 1024]          # NV = 2, 2, 4, 8, 16; 65 / 129 / 257 end in a ragged group
NARROW_V = [2, 29, 64]                      # through the wide entries with one label per lane
KINDS = ["wide", "flat", "const"]
SEED, OFFSET, BOUND, K_MAX = 0xDEADBEEF1234, 3, 2e-6, 16


@functools.lru_cache(maxsize=None)
def sampler_scores(V, kind):
    """tests/test_wide_vocab_gpu.py::_sampler_scores: (40, 8, V) fp32 -- randn * 3, randn * 0.5 or constant rows."""
    g = torch.Generator().manual_seed(V * 7 + len(kind))
    if kind == "const":
        return torch.full((40, 8, V), 0.25)
    return torch.randn(40, 8, V, generator=g) * (3.0 if kind == "wide" else 0.5)


@functools.lru_cache(maxsize=None)
def oracle_draws(V, kind):
    """(paths (16,T,B), cdf (T,B,V), u (16,T,B)) of pg_ref.sample_paths in fp64, read-only."""
    out = pg_ref.sample_paths(sampler_scores(V, kind).numpy(), K_MAX, SEED, OFFSET)
    for a in out:
        a.setflags(write=False)
    return out


def draw_mismatches(s, paths, cdf, u):
    """tests/test_wide_vocab_gpu.py::_sampler_mismatches for draws (K,T,B): a draw may differ from the oracle's only where u lies
    within 2e-6 of the cdf step between the two labels, and at most max(1, draws // 1000) draws may.  Returns (count, the largest
    |cdf - u| at a differing draw)."""
    diff = np.argwhere(s != paths)
    worst = 0.0
    for k, t, b in diff:
        lo = min(s[k, t, b], paths[k, t, b])
        gap = abs(cdf[t, b, lo] - u[k, t, b])
        worst = max(worst, gap)
        assert gap < BOUND, (k, t, b, s[k, t, b], paths[k, t, b], gap)
    assert len(diff) <= max(1, s.size // 1000), len(diff)
    return len(diff), worst


def f32_draws(scores, K):
    """The kernels' rule in plain numpy float32: exp of the differences to the row maximum, a sequential prefix sum, and
    min(#{cdf <= u * total}, V - 1) -- no lanes, no wave scan: what ANY fp32 evaluation of the rule in label order gives."""
    x = np.asarray(scores, dtype=np.float32)
    T, B, V = x.shape
    e = np.exp(x - x.max(axis=2, keepdims=True)).astype(np.float32)
    cdf = np.cumsum(e, axis=2, dtype=np.float32)
    u = pg_ref.sampler_uniforms(T, np.arange(B), K, SEED, OFFSET, B).astype(np.float32)      # 24-bit fractions: exact in fp32
    thr = (u * cdf[None, :, :, -1]).astype(np.float32)
    return np.minimum((cdf[None] <= thr[..., None]).sum(axis=3), V - 1).astype(np.int64)
