"""What test_grad_sync_cpu.py and test_gpu_grad_bucket.py share: the gradient buckets' cases and their numpy restatements.  A plain module."""
import numpy as np

COUNTS = (1, 3, 4, 5, 1023, 65537)                       # 65537: 33 workgroups of 2048 floats, the last one a single quad of one float
MANY = tuple(1 + (7 * i) % 23 for i in range(97))        # 97 tensors: two launches of the 96-entry table
NSRC = (1, 2, 3, 5)
SUM_COUNT = 4 * 600 + 4                                  # 601 quads: three workgroups of 256 threads, the last one ragged
POOL = (1e8, -1e8, 1.0, 2.0 ** -20, 3.0)                 # float32 values whose sum depends on the order


def layout(counts):
    """pmp_grad_bucket_floats restated: -> (the bucket's floats, the tensors' offsets)"""
    padded = (np.asarray(counts, np.int64) + 3) // 4 * 4
    return int(padded.sum()), [int(v) for v in np.concatenate([[0], np.cumsum(padded)[:-1]])]


def gradients(counts, seed=11):
    """One float32 array per tensor, no element zero"""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(c) + 3.0).astype(np.float32) for c in counts]


def packed(grads, counts):
    """pmp_grad_pack_device restated: grads[i] None = a slice of +0.0 -> the bucket"""
    total, offsets = layout(counts)
    out = np.zeros(total, np.float32)
    for g, o, c in zip(grads, offsets, counts):
        if g is not None:
            out[o:o + c] = g
    return out


def sources(nsrc, count=SUM_COUNT, seed=5):
    """nsrc float32 arrays: per element a permutation of 1e8, -1e8, 1, 2^-20 (and, for a fifth source, 3), source j taking the
    permutation's entry j"""
    rng = np.random.default_rng(seed)
    width = max(nsrc, 4)
    pool = np.asarray(POOL[:width], np.float32)
    perm = np.argsort(rng.random((count, width)), axis=1)
    return [np.ascontiguousarray(pool[perm[:, j]]) for j in range(nsrc)]


def ordered_sum(src):
    """((src[0] + src[1]) + src[2]) + ...: float32 additions, each rounded on its own"""
    acc = src[0].astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        for s in src[1:]:
            acc = (acc + s.astype(np.float32)).astype(np.float32)
    return acc
