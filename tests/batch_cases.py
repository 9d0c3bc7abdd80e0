"""The cases of pmp_batch_gather_device (include/pmp.h, TRAINING STEP) and its restatement in numpy, for test_batch_cases_cpu.py and
test_gpu_batch_gather.py: a seeded set of N blocks with its three label arrays, the index lists, and what Metrics.Load_Pre_VP_Dataset's
statements (Metrics.py:78-95, 134-135) make of the same rows.  A plain module."""
import numpy as np

N = 7
KEYS = ("x", "qt_f", "qt8", "msbt", "msdire")


def dataset(n=N, seed=3):
    """-> {"y" u8[n,68,68], "u", "v" u8[n,34,34], "qt8" u8[n,8,8] raw qtDepth (with zeros, which wrap to 255), "msbt" u8[n,3,16,16],
    "msdire" i8[n,3,16,16]}: every byte value occurs in the pixels"""
    rng = np.random.default_rng(seed)
    d = {"y": rng.integers(0, 256, (n, 68, 68), dtype=np.uint8), "u": rng.integers(0, 256, (n, 34, 34), dtype=np.uint8),
         "v": rng.integers(0, 256, (n, 34, 34), dtype=np.uint8), "qt8": rng.integers(0, 5, (n, 8, 8), dtype=np.uint8),
         "msbt": rng.integers(0, 4, (n, 3, 16, 16), dtype=np.uint8), "msdire": rng.integers(-1, 2, (n, 3, 16, 16)).astype(np.int8)}
    d["qt8"][0, 0, 0] = 0
    d["y"][0, 0, :4] = [0, 255, 1, 254]
    return d


def indices():
    """name -> int64 index list over N rows: one row, five with a repeat, 257 (more rows than a workgroup has threads)"""
    rng = np.random.default_rng(11)
    return {"n1": np.array([4], np.int64), "n5": np.array([6, 0, 3, 0, 5], np.int64), "n257": rng.integers(0, N, 257).astype(np.int64)}


def gather(d, index, chroma):
    """The restatement: -> ({x, qt_f, qt8, msbt, msdire}, status).  A row whose index is outside [0, N) is zeros and sets bit 0."""
    index = np.asarray(index, np.int64)
    n, ok = d["y"].shape[0], (index >= 0) & (index < d["y"].shape[0])
    at = np.where(ok, index, 0)
    y = d["y"][at]
    if chroma:
        pooled = y.reshape(-1, 34, 2, 34, 2).max(axis=(2, 4))
        x = np.stack([pooled, d["u"][at], d["v"][at]], 1).astype(np.float32)
    else:
        x = y[:, None].astype(np.float32)
    out = {"x": x, "qt_f": (d["qt8"][at] - np.uint8(1)).astype(np.uint8)[:, None].astype(np.float32), "qt8": d["qt8"][at].copy(),
           "msbt": d["msbt"][at].copy(), "msdire": d["msdire"][at].copy()}
    for a in out.values():
        a[~ok] = 0
    assert n >= 1
    return out, int((~ok).any())


def loader_rows(d, index, chroma):
    """What Load_Pre_VP_Dataset's statements build, on the CPU with torch, for the rows `index` (all in range) -> {x, qt_f, msbt, msdire}"""
    import torch
    import torch.nn.functional as F
    input_batch = torch.FloatTensor(np.expand_dims(d["y"], 1))
    if chroma:
        input_batch = F.max_pool2d(input_batch, 2)
        input_batch1 = torch.FloatTensor(np.expand_dims(d["u"], 1))
        input_batch2 = torch.FloatTensor(np.expand_dims(d["v"], 1))
        input_batch = torch.cat([input_batch, input_batch1, input_batch2], 1)
    qt_label_batch = torch.FloatTensor(np.expand_dims(d["qt8"], 1) - 1)
    bt_label_batch = torch.FloatTensor(d["msbt"])
    dire_label_batch = torch.FloatTensor(d["msdire"])
    at = torch.from_numpy(np.asarray(index, np.int64))
    return {"x": input_batch[at].numpy(), "qt_f": qt_label_batch[at].numpy(), "msbt": bt_label_batch[at].numpy(),
            "msdire": dire_label_batch[at].numpy()}
