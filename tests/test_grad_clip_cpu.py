"""Gradient clipping by global norm on a GPU-less host: the new entry points are exported, bound with the header's argument
counts and reject invalid arguments before any device work; ``max_grad_norm`` is validated; and the CPU plumbing path of
``DataParallelStep`` (torch's Adam, gloo) follows the device's rule -- scale = min(1, max / (norm + 1e-6)) over the REDUCED
gradient, a non-finite gradient skips the update on every rank -- against a hand-written ``clip_grad_norm_`` loop."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from policy_gradient_asr_amd.train_step import FLAG_PAD, shard_slice
from test_dp_gloo_cpu import ToyStep, ToyStepTwoBuckets, _free_port, make_data, make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_grad_norm_ws_bytes", "pgasr_grad_norm_clip", "pgasr_adam_step_clipped")
INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_clip_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib, hipops
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["pgasr_grad_norm_clip"][0] is ctypes.c_int
    assert _lib.SIGNATURES["pgasr_adam_step_clipped"][0] is ctypes.c_int
    assert _lib.SIGNATURES["pgasr_grad_norm_ws_bytes"][0] is ctypes.c_size_t
    # one argument more than the unclipped update: the clip state
    assert len(_lib.SIGNATURES["pgasr_adam_step_clipped"][1]) == len(_lib.SIGNATURES["pgasr_adam_step"][1]) + 1
    assert lib.pgasr_abi_version() == 7 and int(re.search(r"#define PGASR_ABI_VERSION (\d+)", raw).group(1)) == 7
    assert int(re.search(r"#define PGASR_CLIP_STATE_BYTES (\d+)", raw).group(1)) == 4 * hipops.CLIP_STATE_WORDS


def test_workspace_query(lib):
    assert lib.pgasr_grad_norm_ws_bytes(0) == 0
    assert lib.pgasr_grad_norm_ws_bytes(1) == 8                          # one workgroup, one fp64 partial
    assert lib.pgasr_grad_norm_ws_bytes(1024) == 8 and lib.pgasr_grad_norm_ws_bytes(1025) == 16
    big = lib.pgasr_grad_norm_ws_bytes(4_787_549)
    assert big == lib.pgasr_grad_norm_ws_bytes(1 << 40) == 8192          # the grid is capped: the workspace never grows beyond 8 KB


def test_invalid_arguments_are_rejected_without_a_device(lib):
    """Every call below returns PGASR_ERR_INVALID_ARG before anything is launched (the pointers are never dereferenced)."""
    p, n = 0x1000, 1000
    need = lib.pgasr_grad_norm_ws_bytes(n)
    assert lib.pgasr_grad_norm_clip(p, 0, 1.0, p, need, p, None) == INVALID_ARG              # n = 0
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert lib.pgasr_grad_norm_clip(p, n, bad, p, need, p, None) == INVALID_ARG, bad      # max_norm not > 0
    assert lib.pgasr_grad_norm_clip(p + 4, n, 1.0, p, need, p, None) == INVALID_ARG          # gradient not 16-byte aligned
    assert lib.pgasr_grad_norm_clip(p, n, 1.0, p + 4, need, p, None) == INVALID_ARG          # workspace not 8-byte aligned
    assert lib.pgasr_grad_norm_clip(p, n, 1.0, p, need, p + 8, None) == INVALID_ARG          # state not 16-byte aligned
    assert lib.pgasr_grad_norm_clip(p, n, 1.0, p, need - 1, p, None) == INVALID_ARG          # workspace too small
    assert lib.pgasr_grad_norm_clip(p, 1 << 20, 1.0, p, need, p, None) == INVALID_ARG        # .. for this n
    for args in ((None, n, 1.0, p, need, p), (p, n, 1.0, None, need, p), (p, n, 1.0, p, need, None)):
        assert lib.pgasr_grad_norm_clip(*args, None) == INVALID_ARG                          # null pointers
    adam = (p, p, p, p, n, 1, 5e-4, 0.9, 0.999, 1e-8, 0.0, None, None, None)
    assert lib.pgasr_adam_step_clipped(*adam, None, None) == INVALID_ARG                     # no clip state
    assert lib.pgasr_adam_step_clipped(*adam, p + 4, None) == INVALID_ARG                    # misaligned clip state
    assert lib.pgasr_adam_step_clipped(p, p, p, p, 0, 1, 5e-4, 0.9, 0.999, 1e-8, 0.0, None, None, None, p, None) == INVALID_ARG


def test_hipops_clip_calls_refuse_cpu_tensors():
    from policy_gradient_asr_amd import _lib, hipops
    with pytest.raises(_lib.PgasrError):
        hipops.grad_norm_clip(torch.ones(8), 1.0)
    z = torch.zeros(8)
    with pytest.raises(_lib.PgasrError):
        hipops.adam_step(z, z, z, z, 1, clip_state=torch.zeros(8))


def test_max_grad_norm_is_validated_in_the_constructor():
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    for ok in (None, 1.0, 3, 1e-3, float("inf")):
        st = ToyStep(make_model(), lr=1e-2, max_grad_norm=ok)
        assert st.max_grad_norm == (None if ok is None else float(ok))
        assert st.clip_counts() == (0, 0)
    for bad in (True, False, 0, 0.0, -1.0, float("nan"), float("-inf"), "1.0", [1.0]):
        with pytest.raises(ValueError):
            ToyStep(make_model(), lr=1e-2, max_grad_norm=bad)
        with pytest.raises(ValueError):
            PolicyGradientTrainer(make_model(), max_grad_norm=bad)


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


def _reference_loop(max_norm, steps=5):
    """loss.backward(); clip_grad_norm_(params, max_norm); Adam.step() -- what a user of the reference writes."""
    model = make_model()
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    x, y = make_data()
    out = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((model(x) - y) ** 2).sum() / x.shape[0]
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        opt.step()
        out.append((_flat(params).clone(), _flat([opt.state[p]["exp_avg"] for p in params]).clone(), norm))
    return out


@pytest.mark.parametrize("max_norm,clipped", [(2.0, [True, True, False, False, False]), (1.0, [True] * 5)])
def test_clipped_steps_match_a_torch_loop(max_norm, clipped):
    """The toy model's unclipped norms over five steps are 2.20, 2.07, 1.95, 1.84, 1.74: a bound of 2.0 clips the first two steps
    and no other, a bound of 1.0 all five.  Parameters AND Adam's first moment (linear in the scale, unlike the nearly
    scale-invariant update) equal the torch loop's after every step."""
    ref = _reference_loop(max_norm)
    st = ToyStep(make_model(), lr=1e-2, max_grad_norm=max_norm)
    x, y = make_data()
    norms = []
    for i in range(5):
        st.step(x, y)
        norms.append(float(st.last_grad_norm))
        print(f"step {i + 1}: norm {norms[-1]:.6f} (torch loop {ref[i][2]:.6f})")
        torch.testing.assert_close(st.flat[FLAG_PAD:], ref[i][0], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(st.opt.state[st.flat_param]["exp_avg"][FLAG_PAD:], ref[i][1], rtol=1e-5, atol=1e-9)
        assert norms[-1] == pytest.approx(ref[i][2], rel=1e-5)
        # gflat keeps the UNCLIPPED reduced gradient (Adam reads scale * g): its norm is the recorded one
        assert float(st.gflat[FLAG_PAD:].double().norm()) == pytest.approx(norms[-1], rel=1e-6)
    assert [n > max_norm for n in norms] == clipped, norms
    assert st.clip_counts() == (sum(clipped), 0)
    assert st.applied_steps() == 5


def test_an_infinite_bound_gives_the_bits_of_no_bound():
    runs = []
    for bound in (None, float("inf")):
        st = ToyStep(make_model(), lr=1e-2, max_grad_norm=bound)
        x, y = make_data()
        snaps = []
        for _ in range(5):
            st.step(x, y)
            snaps.append(st.flat.clone())
        runs.append((snaps, st))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert runs[0][1].last_grad_norm is None and runs[0][1].clip_counts() == (0, 0)
    assert math.isfinite(float(runs[1][1].last_grad_norm)) and runs[1][1].clip_counts() == (0, 0)


def _worker_clip(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ToyStepTwoBuckets(make_model(), lr=1e-2, world_size=world, max_grad_norm=1.0)
        x, y = make_data()
        sl = shard_slice(8, rank, world)
        norms = []
        for _ in range(3):
            st.step(x[sl], y[sl])
            norms.append(float(st.last_grad_norm))
        q.put((rank, st.flat.tolist(), norms, st.clip_counts()))
    finally:
        dist.destroy_process_group()


def _spawn(target, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def test_two_gloo_ranks_clip_by_the_norm_of_the_summed_gradient():
    res = _spawn(_worker_clip)
    st = ToyStep(make_model(), lr=1e-2, max_grad_norm=1.0)
    x, y = make_data()
    want_norms = []
    for _ in range(3):
        st.step(x, y)
        want_norms.append(float(st.last_grad_norm))
    assert res[0][1] == res[1][1]                                  # replicas bit-identical after three clipped steps
    assert res[0][2] == res[1][2]                                  # both ranks measured the same (reduced) gradient
    for rank, flat, norms, counts in res:
        torch.testing.assert_close(torch.tensor(flat), st.flat, rtol=1e-5, atol=1e-6)
        assert norms == pytest.approx(want_norms, rel=1e-5)        # the norm of the SUM, not of the rank's shard
        assert counts == (3, 0)


class ToyStepOneRankOverflows(ToyStepTwoBuckets):
    """Rank 1's loss overflows in its SECOND step only: its gradient is inf / NaN, the all-reduce carries that to every rank,
    and the non-finite guard of every rank skips the update."""

    def forward_loss(self, batch, global_batch):
        loss = super().forward_loss(batch, global_batch)
        if dist.get_rank() == 1 and self.nstep == 1:
            loss = loss * float("inf")
        return loss


def _worker_nonfinite(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ToyStepOneRankOverflows(make_model(), lr=1e-2, world_size=world, max_grad_norm=1.0)
        x, y = make_data()
        sl = shard_slice(8, rank, world)
        snaps, norms = [], []
        for _ in range(3):
            st.step(x[sl], y[sl])
            snaps.append(st.flat.tolist())
            norms.append(float(st.last_grad_norm))
        q.put((rank, snaps, norms, st.applied_steps(), st.nstep, st.clip_counts()))
    finally:
        dist.destroy_process_group()


def test_a_non_finite_gradient_on_one_rank_skips_the_update_on_every_rank():
    res = _spawn(_worker_nonfinite)
    for rank, snaps, norms, applied, calls, counts in res:
        assert calls == 3 and applied == 2, (rank, calls, applied)
        assert snaps[1] == snaps[0]                                # the overflowing step changed nothing, on the other rank too
        assert snaps[2] != snaps[1]                                # the next step is applied again
        assert all(math.isfinite(v) for v in snaps[2])
        assert math.isfinite(norms[0]) and not math.isfinite(norms[1]) and math.isfinite(norms[2])
        assert counts == (2, 1)
    assert res[0][1] == res[1][1]                                  # replicas bit-identical after every step
