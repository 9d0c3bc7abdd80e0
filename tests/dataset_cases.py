"""Inputs behind tests/golden/g21_dataset.npz (CreateDataSet.output_block_yuv) and the data set assembly tests: seeded YUV files, a numpy
restatement of the block cutter with temporal sub-sampling, of pmp_select_rows_device and of pmp_gather_rows_device, and the case lists
of tests/test_gpu_dataset.py.

The fixture holds outputs only.  Its input is rebuilt here from a seed, so that tools/gen_golden_dataset.py (which runs the reference
on it) and the tests see the same bytes.  Not a test module: no test_ prefix."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_dataset.npz")

# the golden's sequence: sides that are no multiples of 64, 33 frames at ratio 8 = frames 0, 8, 16, 24, 32: 5 x (2 x 3) = 30 blocks,
# the fewest output_block_yuv survives (it plots block_v[29])
G21 = dict(width=192, height=136, frames=33, ss=8, seed=2101)      # three block columns, two block rows and a remainder of 8 lines


# ------------------------------------------------------------------------------------------------ YUV files
def yuv_planes(width, height, frames, bits, seed):
    """Seeded planes y[F,H,W], u, v[F,H/2,W/2], u8 or (10 bits) u16 with every value 0..1023 likely; the first samples of frame 0
    are the half-even and clip cases of round(x / 4)."""
    rng = np.random.default_rng(seed + bits)
    dt, top = (np.uint8, 256) if bits == 8 else (np.uint16, 1024)
    y = rng.integers(0, top, (frames, height, width)).astype(dt)
    u = rng.integers(0, top, (frames, height // 2, width // 2)).astype(dt)
    v = rng.integers(0, top, (frames, height // 2, width // 2)).astype(dt)
    if bits == 10:
        y[0, 0, :8] = [2, 6, 10, 14, 1021, 1022, 1023, 1018]
    return y, u, v


def write_yuv(path, width, height, frames, bits, seed):
    """The planar 4:2:0 file of yuv_planes -> the planes"""
    y, u, v = yuv_planes(width, height, frames, bits, seed)
    with open(path, "wb") as fp:
        for i in range(frames):
            fp.write(y[i].tobytes()); fp.write(u[i].tobytes()); fp.write(v[i].tobytes())
    return y, u, v


# ------------------------------------------------------------------------------------------------ restatements
def cut(y, u, v, bits, ss=1):
    """CreateDataSet.output_block_yuv (:89-141) on planes, frames range(0, F, ss): 10-bit samples become round-half-even(x / 4)
    clipped to 255; every plane is padded top and left by the overlap (4, chroma 2) and cut into 68x68 / 34x34 windows, frame-major,
    row-major, the right and bottom remainders dropped -> by u8[n,68,68], bu, bv u8[n,34,34]"""
    out = []
    bh, bw = y.shape[1] // 64, y.shape[2] // 64
    for plane, bs, ov in ((y, 64, 4), (u, 32, 2), (v, 32, 2)):
        p = plane[::ss]
        if bits == 10:
            p = np.round(p / 4).clip(0, 255)
        p = p.astype(np.uint8)
        pad = np.zeros((p.shape[0], p.shape[1] + ov, p.shape[2] + ov), np.uint8)
        pad[:, ov:, ov:] = p
        blocks = [pad[f, i * bs:(i + 1) * bs + ov, j * bs:(j + 1) * bs + ov] for f in range(p.shape[0]) for i in range(bh) for j in range(bw)]
        out.append(np.array(blocks, np.uint8).reshape(len(blocks), bs + ov, bs + ov))
    return tuple(out)


def block_rows(seqs, ss):
    """[(width, height, frames)] in table order -> i64[n,4]: (sequence, sub-sampled frame, block row, block column) of every row"""
    rows = []
    for si, (w, h, f) in enumerate(seqs):
        for k in range((f + ss - 1) // ss):
            for i in range(h // 64):
                for j in range(w // 64):
                    rows.append((si, k, i, j))
    return np.array(rows, np.int64).reshape(-1, 4)


def select(flags, mask, seg_end, cap, n):
    """pmp_select_rows_device in plain loops -> (index i64[n] with its -1 tail, count i64[nseg + 1])"""
    index = np.full(n, -1, np.int64)
    count = np.zeros(len(seg_end) + 1, np.int64)
    m, start = 0, 0
    for s, end in enumerate(seg_end):
        seen = 0
        for i in range(start, int(end)):
            if all((int(f[i]) & mask) == 0 for f in flags):
                if cap == 0 or seen < cap:
                    index[m] = i
                    m += 1
                    count[s] += 1
                seen += 1
        start = int(end)
    count[-1] = m
    return index, count


def gather(src, index):
    """pmp_gather_rows_device -> (rows, status): an index outside the source gives a row of zeros and status 1"""
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < len(src))
    out = np.zeros((len(index),) + src.shape[1:], src.dtype)
    out[ok] = src[index[ok]]
    return out, int(not ok.all())


# ------------------------------------------------------------------------------------------------ the cases of test_gpu_dataset.py
SELECT_N = (1, 63, 64, 65, 255, 256, 257, 1025, 4097)     # wave, workgroup, tile and grid boundaries of the scan
SELECT_CAPS = (0, 1, 5, 1 << 20)
FLAG_PATTERNS = ("none", "all", "alternating", "random", "last")
GATHER_ROW_BYTES = (4, 64, 256, 768, 1156, 4624)
GATHER_M = (1, 65, 1025)


def flag_arrays(pattern, nflags, n, seed):
    """nflags arrays u8[n] whose bits 0 and 2 the mask 5 looks at follow `pattern`; bit 1 (PMP_MSBT_QT_DEEP), which the mask ignores,
    is set at random everywhere"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(nflags):
        noise = (rng.random(n) < 0.5).astype(np.uint8) * 2
        if pattern == "none":
            f = np.zeros(n, np.uint8)
        elif pattern == "all":
            f = np.full(n, 1 if k % 2 == 0 else 4, np.uint8)
        elif pattern == "alternating":
            f = ((np.arange(n) + k) % 2).astype(np.uint8) * (4 if k == 1 else 1)
        elif pattern == "random":
            f = (rng.random(n) < 0.5 ** (1.0 / nflags)).astype(np.uint8)      # the rows clear in every array: about half
            f = (1 - f) * rng.choice(np.array([1, 4, 5], np.uint8), n)
        else:
            f = np.zeros(n, np.uint8)
            f[-1] = 5
        out.append((f | noise).astype(np.uint8))
    return out


def segment_lists(n):
    """{name: seg_end} of the segment cases at n rows"""
    segs = {"one": [n], "each_row": list(range(1, n + 1))}
    if n >= 3:
        a, b = max(1, n // 3), max(2, (2 * n) // 3 + (1 if n > 70 else 0))        # ends inside a wave, not on a boundary
        segs["inside_wave"] = [a, b, n]
        segs["empty_first_middle_last"] = [0, 0, a, a, a, b, n, n]
    return segs
