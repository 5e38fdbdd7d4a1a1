"""Gradient accumulation over micro-batches on a GPU-less host: the rules of ``DataParallelStep.step_accumulated`` /
``accumulate_gradients`` on the toy model of tests/test_dp_gloo_cpu.py (one process and two gloo ranks), the id-addressed sampler
entry points' export / binding / argument checks (no compute calls), the host-side id checks, and the default id rule."""
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from policy_gradient_asr_amd.train_step import (FLAG_PAD, DataParallelStep, check_utt_ids, default_utt_ids, shard_slice)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_frame_argmax_sample_ids", "pgasr_frame_sample_multi_ids")
INVALID_ARG, UNSUPPORTED = 1, 4


class ToyStep(DataParallelStep):
    def forward_loss(self, batch, global_batch):
        x, y = batch
        self.seen.append((self._micro.index if self._micro is not None else None, global_batch, self.nstep))
        return ((self.model(x) - y) ** 2).sum() / global_batch

    seen = early = None


class ToyStepTwoBuckets(ToyStep):
    """The N>1 trainer's bucket split; inside an accumulated step only the LAST micro-batch's call starts a collective."""

    def backward(self, loss):
        loss.backward()
        self.reduce_upper(self.param_offset("2.weight"))
        self.early.append(self._early is not None)         # did this call start the upper bucket's all-reduce?


class ToyStepOneRankFails(ToyStepTwoBuckets):
    """Rank 1 reports invalid gradients in its SECOND accumulated step only."""
    fail_rank, fail_call = 1, 1
    flag_writes = 0

    def write_local_error_flag(self):
        assert float(self.gflat[0]) == 0.0           # no micro-batch disturbed the flag word before it is written
        bad = dist.get_rank() == self.fail_rank and self.nstep == self.fail_call
        self.gflat[0] = 1.0 if bad else 0.0
        self.flag_writes += 1
        return True


def make_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def make_data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(8, 6, generator=g), torch.randn(8, 3, generator=g)


def make_step(cls=ToyStep, **kw):
    st = cls(make_model(), lr=1e-2, **kw)
    st.seen, st.early = [], []
    return st


def split(x, y, sizes):
    out, o = [], 0
    for n in sizes:
        out.append((x[o:o + n], y[o:o + n]))
        o += n
    return out


@pytest.mark.parametrize("sizes", [(4, 4), (3, 5), (1, 1, 6)])
def test_accumulated_micro_batches_give_the_whole_batch(sizes):
    x, y = make_data()
    whole = make_step()
    ref_loss = float(whole.compute_gradients(x, y))
    acc = make_step()
    loss = acc.accumulate_gradients(split(x, y, sizes))
    assert not loss.requires_grad
    torch.testing.assert_close(acc.gflat, whole.gflat, rtol=1e-5, atol=1e-6)
    assert float(loss) == pytest.approx(ref_loss, rel=1e-5)
    assert acc.nstep == 0 and acc.applied_steps() == 0                      # no update, no step counted
    # every micro-batch was normalised by the whole batch and saw the same step number; their indices travel as instance state
    assert acc.seen == [(j, 8, 0) for j in range(len(sizes))]
    assert acc._micro is None and not acc._hold_collectives

    # one optimizer update, equal to the whole batch's
    ref_loss = float(whole.step(x, y))
    before = acc.flat.clone()
    loss = acc.step_accumulated(split(x, y, sizes))
    assert acc.nstep == 1 and acc.applied_steps() == 1
    assert not torch.equal(acc.flat, before)
    torch.testing.assert_close(acc.flat, whole.flat, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(acc.gflat, whole.gflat, rtol=1e-5, atol=1e-6)
    assert float(loss) == pytest.approx(ref_loss, rel=1e-5)
    # gflat is zeroed once per accumulated step, not carried over from the call before
    acc.accumulate_gradients(split(x, y, sizes))
    whole.compute_gradients(x, y)
    torch.testing.assert_close(acc.gflat, whole.gflat, rtol=1e-5, atol=1e-6)


def test_one_micro_batch_is_the_plain_step():
    x, y = make_data()
    a, b = make_step(), make_step()
    la, lb = a.step(x, y), b.step_accumulated([(x, y)])
    assert torch.equal(a.flat, b.flat) and torch.equal(a.gflat, b.gflat) and torch.equal(la, lb)
    assert a.nstep == b.nstep == 1
    # step(utt_ids=) is the one-micro-batch accumulated step
    c = make_step()
    lc = c.step(x, y, utt_ids=[7, 6, 5, 4, 3, 2, 1, 0])
    assert torch.equal(a.flat, c.flat) and torch.equal(la, lc) and c.nstep == 1
    c.compute_gradients(x, y, utt_ids=list(range(8)))
    assert c.nstep == 1


def test_clip_acts_once_on_the_accumulated_gradient():
    x, y = make_data()
    whole, acc = make_step(max_grad_norm=0.05), make_step(max_grad_norm=0.05)
    whole.step(x, y)
    acc.step_accumulated(split(x, y, (3, 5)))
    assert acc.clip_counts() == whole.clip_counts() == (1, 0)
    assert float(acc.last_grad_norm) == pytest.approx(float(acc.gflat[FLAG_PAD:].double().norm()), rel=1e-6)
    torch.testing.assert_close(acc.flat, whole.flat, rtol=1e-5, atol=1e-6)


def test_argument_checks_without_a_device():
    x, y = make_data()
    st = make_step()
    mbs = split(x, y, (4, 4))
    with pytest.raises(ValueError):
        st.step_accumulated([])
    with pytest.raises(ValueError):
        st.accumulate_gradients([])
    with pytest.raises(ValueError):
        st.step_accumulated([mbs[0], (x[:0], y[:0])])                                  # an empty micro-batch
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [4, 5, 6, 4]])                 # a duplicate inside one micro-batch
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [3, 5, 6, 7]])                 # .. and across two
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [4, 5, 6, 8]])                 # out of range
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [4, 5, 6, -1]])
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [4, 5, 6]])                    # a wrong count for a micro-batch
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3]])                               # fewer id lists than micro-batches
    with pytest.raises(ValueError):
        st.step_accumulated(mbs, utt_ids=[[0, 1, 2, 3], [4, 5, 6, 7.5]])               # not an integer
    with pytest.raises(ValueError):
        st.step(x, y, utt_ids=[0, 1, 2, 3, 4, 5, 6, 6])
    assert st.nstep == 0 and st.applied_steps() == 0 and st._micro is None            # nothing ran
    # the lock was released by every failure
    st.step_accumulated(mbs, utt_ids=[[7, 5, 3, 1], [0, 2, 4, 6]])
    assert st.nstep == 1
    assert check_utt_ids([(1, 0), torch.tensor([2])], (2, 1), 1) == [[1, 0], [2]]
    assert check_utt_ids([[5], [0]], (1, 1), 3) == [[5], [0]]                          # the range is world x the step's utterances


def test_loss_rejects_two_addressings_without_a_device():
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        pg_ctc_loss(z, il, tg, tl, global_batch=4, sample_ids=torch.tensor([2, 3], dtype=torch.int32), sample_base=0)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_default_ids_are_a_bijection_onto_the_global_batch(world):
    sizes = (16, 16, 7)
    ids = [default_utt_ids(sizes, r, world) for r in range(world)]
    for r in range(world):
        assert [len(m) for m in ids[r]] == list(sizes)
    flat = [i for per_rank in ids for m in per_rank for i in m]
    assert sorted(flat) == list(range(world * sum(sizes)))
    # micro-batch j is a contiguous slice of the global batch, sharded contiguously over the ranks
    off = 0
    for j, n in enumerate(sizes):
        assert [i for r in range(world) for i in ids[r][j]] == list(range(world * off, world * (off + n)))
        off += n
    check_utt_ids(ids[0], sizes, world)


# ---- the id-addressed sampler entry points ----
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_id_sampler_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 11 and len(_lib.SIGNATURES[NEW[1]][1]) == 12
    assert lib.pgasr_abi_version() == 7 and int(re.search(r"#define PGASR_ABI_VERSION (\d+)", raw).group(1)) == 7


def test_id_sampler_argument_checks_need_no_device(lib):
    """Every rejection below happens before a launch: the pointers are never dereferenced."""
    p = 0x1000
    one, multi = lib.pgasr_frame_argmax_sample_ids, lib.pgasr_frame_sample_multi_ids
    assert one(p, 10, 2, 29, 0, 0, 4, None, p, p, None) == INVALID_ARG               # NULL ids
    assert multi(p, 10, 2, 29, 4, 0, 0, 4, None, None, p, None) == INVALID_ARG
    assert one(p, 10, 2, 29, 0, 0, 0, p, p, p, None) == INVALID_ARG                  # ctr_stride = 0: no "0 means B" here
    assert multi(p, 10, 2, 29, 4, 0, 0, 0, p, None, p, None) == INVALID_ARG
    assert one(p, 10, 2, 29, 0, 0, -3, p, p, p, None) == INVALID_ARG
    for K in (0, 17):
        assert multi(p, 10, 2, 29, K, 0, 0, 4, p, None, p, None) == INVALID_ARG
    assert one(p, 10, 2, 65, 0, 0, 4, p, p, p, None) == UNSUPPORTED                  # V > 64
    assert multi(p, 10, 2, 65, 4, 0, 0, 4, p, None, p, None) == UNSUPPORTED
    # T * ctr_stride > 2^32: counter word 0 is 32 bits
    assert one(p, 4096, 2, 29, 0, 0, (1 << 20) + 1, p, p, p, None) == UNSUPPORTED
    assert multi(p, 4096, 2, 29, 4, 0, 0, (1 << 20) + 1, p, None, p, None) == UNSUPPORTED
    assert one(p, 4096, 2, 29, 0, 0, 1 << 20, p, None, None, None) == 0              # exactly 2^32 counters fit (nothing to write: no launch)


# ---- two gloo ranks, two micro-batches each ----
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _count_all_reduces():
    calls = []
    real = dist.all_reduce

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counted
    return calls


def _rank_micro_batches(rank, world):
    """The 8 samples as two micro-batches of 4, each sharded contiguously over the ranks (``default_utt_ids``)."""
    x, y = make_data()
    out = []
    for j in range(2):
        sl = shard_slice(4, rank, world)
        out.append((x[4 * j:4 * j + 4][sl], y[4 * j:4 * j + 4][sl]))
    return out


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model = make_model()
        if rank == 1:
            with torch.no_grad():
                for p in model.parameters():
                    p.add_(1.0)
        st = ToyStepTwoBuckets(model, lr=1e-2, world_size=world)
        st.seen, st.early = [], []
        calls = _count_all_reduces()
        mbs = _rank_micro_batches(rank, world)
        losses, per_step = [], []
        for _ in range(3):
            n0 = len(calls)
            losses.append(float(st.step_accumulated(mbs)))
            per_step.append(len(calls) - n0)
        n0 = len(calls)
        st.accumulate_gradients(mbs)
        q.put((rank, st.flat.tolist(), losses, per_step, len(calls) - n0, st.seen, st.nstep, st.applied_steps(), st.early))
    finally:
        dist.destroy_process_group()


def _worker_flag(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ToyStepOneRankFails(make_model(), lr=1e-2, world_size=world)
        st.seen, st.early = [], []
        mbs = _rank_micro_batches(rank, world)
        snaps = []
        for _ in range(3):
            st.step_accumulated(mbs)
            snaps.append(st.flat.tolist())
        q.put((rank, snaps, st.applied_steps(), st.nstep, st.flag_writes))
    finally:
        dist.destroy_process_group()


def _run(target, world=2):
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


def test_two_gloo_ranks_two_micro_batches_each():
    res = _run(_worker)
    st = make_step()
    x, y = make_data()
    ref_losses = [float(st.step(x, y)) for _ in range(3)]
    for rank, flat, losses, per_step, in_accumulate, seen, nstep, applied, early in res:
        torch.testing.assert_close(torch.tensor(flat), st.flat, rtol=1e-5, atol=1e-6)      # the whole batch's three updates
        assert per_step == [2, 2, 2], per_step        # one all-reduce sequence (two buckets) per accumulated step, not per micro-batch
        assert in_accumulate == 0                     # accumulate_gradients exchanges nothing
        # the early bucket goes out during the LAST micro-batch's backward only (never in accumulate_gradients)
        assert early == [False, True] * 3 + [False, False]
        assert nstep == 3 and applied == 3
        # global_batch = world x the rank's utterances over the step
        assert seen[:2] == [(0, 8, 0), (1, 8, 0)]
    for i in range(3):
        assert res[0][2][i] + res[1][2][i] == pytest.approx(ref_losses[i], rel=1e-5)
    assert res[0][1] == res[1][1]                     # replicas bit-identical


def test_two_gloo_ranks_gradient_is_the_whole_batch():
    """gflat after the exchange of an accumulated step = the single-process whole-batch gradient."""
    res = _run(_worker_grad)
    st = make_step()
    x, y = make_data()
    st.compute_gradients(x, y)
    for rank, gflat in res:
        torch.testing.assert_close(torch.tensor(gflat), st.gflat, rtol=1e-5, atol=1e-6)
    assert res[0][1] == res[1][1]


def _worker_grad(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ToyStepTwoBuckets(make_model(), lr=1e-2, world_size=world)
        st.seen, st.early = [], []
        st.step_accumulated(_rank_micro_batches(rank, world))
        q.put((rank, st.gflat.tolist()))
    finally:
        dist.destroy_process_group()


def test_error_flag_of_an_accumulated_step_skips_the_update_on_every_rank():
    res = _run(_worker_flag)
    for rank, snaps, applied, calls, flag_writes in res:
        assert calls == 3 and applied == 2, (rank, calls, applied)
        assert flag_writes == 3                       # once per accumulated step, after the last micro-batch
        assert snaps[1] == snaps[0]                   # the flagged step changed nothing on either rank
        assert snaps[2] != snaps[1]
    assert res[0][1] == res[1][1]
