"""One rank of test_grad_sync_cpu.py's two-rank gloo jobs on the CPU (started by parallel.spawn_ranks; no GPU): the gathers of
grad_sync.py on CPU tensors and train_qbd's desync check.  argv[1]: "agree" or "apart" (rank 1's parameters differ).  A plain script."""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from pmp_vvc_tip2023_amd import grad_sync as G, parallel, train_qbd as T  # noqa: E402


def main():
    rank, world, _ = parallel.init_process_group(None)
    cpu = torch.device("cpu")
    every = G.all_gather_rows(torch.arange(3, dtype=torch.float64) + 10 * rank)
    assert every.tolist() == [[10.0 * r + i for i in range(3)] for r in range(world)]
    # three batches dealt out to two ranks: 2 and 1; the rows come back in batch order, the sizes beside them
    counts = parallel.shard_counts(3, world)
    lo, _ = parallel.shard_bounds(3, rank, world)
    S = np.arange(counts[rank] * 20, dtype=np.float64).reshape(-1, 20) + 1000 * lo + 0.1
    S_all, ns = G.gather_batch_stats(S, [5 + lo + i for i in range(counts[rank])], counts, cpu)
    assert S_all.shape == (3, 20) and ns == [5, 6, 7], (S_all.shape, ns)
    assert S_all[0, 0] == 0.1 and S_all[1, 0] == 20.1 and S_all[2, 0] == 2000.1, S_all[:, 0]
    fp = 0xFEDCBA9876543210 if sys.argv[1] == "agree" or rank != 1 else 0xFEDCBA9876543211
    trainer = types.SimpleNamespace(fingerprint=lambda: fp, device=cpu, sync=types.SimpleNamespace(rank=rank))
    ok = T.in_sync(trainer, "after epoch 3")
    if not ok:
        return T.EXIT_DESYNC
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
