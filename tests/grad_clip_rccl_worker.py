"""One rank of tests/test_grad_clip_gpu.py's two-rank case (not a test module itself): the real trainer with ``max_grad_norm`` on its
own GPU, gradients all-reduced over RCCL in the early-reduce (two-bucket) order.  argv: rank world port out_dir max_grad_norm"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_rccl_worker as w  # noqa: E402  (sets the queue / IPC environment of the RCCL tests, provides make_batch)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def build(dev, world, rank, max_grad_norm, pg=None):
    """dp_rccl_worker.build (lambda = 1) with the clipping bound."""
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    torch.manual_seed(0)
    m = Seq2Seq(29, n_feats=80)
    m.apply(weights)
    if rank == 1:      # replicas start different: the trainer must broadcast rank 0's weights
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.5)
    m = m.to(dev).eval()
    return PolicyGradientTrainer(m, lr=1e-3, lam=1.0, seed=11, world_size=world, rank=rank, process_group=pg,
                                 max_grad_norm=max_grad_norm)


def main():
    rank, world, port, out_dir, bound = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], float(sys.argv[5])
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    from policy_gradient_asr_amd import streams
    streams.prime()          # before the communicator takes its stream from torch's pool
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, device_id=dev)
    try:
        from policy_gradient_asr_amd.train_step import shard_slice
        tr = build(dev, world, rank, bound)
        assert tr.early_reduce and tr.upper_split is not None
        batch = w.make_batch(8 * world, 80, 60, 29, 6)
        sl = shard_slice(8 * world, rank, world)
        mine = [t[sl].to(dev) for t in batch]
        norms = []
        for _ in range(2):
            tr.step(*mine)
            torch.cuda.synchronize()
            norms.append(tr.last_grad_norm.cpu().clone())
        torch.save({"flat": tr.flat.cpu(), "gflat": tr.gflat.cpu(), "norms": torch.stack(norms), "counts": tr.clip_counts(),
                    "applied": tr.applied_steps(), "world": dist.get_world_size()}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
