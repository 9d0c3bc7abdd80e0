"""Generate tests/golden/g10_m2p_params.npz from the IMPORTED REFERENCE: Map2Partition under other thresholds.

Run in the build container only (needs the reference checkout):   python tools/gen_golden_m2p_params.py
For every threshold set of tests/m2p_params_cases.py (SETS) and both chroma factors, the reference's own code runs on the inputs that
module builds (slices of G3 and G9, and direction cells placed at float32(thd) and its neighbours):
    fixed = Metrics.eli_structual_error(qt)
    m = Map2Partition.Map_to_Partition(fixed, bt, dire, cf, lamb1, lamb2, lamb3, lamb4, lamb5)
    m.msdire_map = Map2Partition.th_round(dire, thd=thd)          # __init__ calls it with 0.5 (Map2Partition.py:105)
    hor, ver = m.get_partition()[0][:, :16, :16]; dout = ...     # as map_to_parititon crops them (:368-373)
and one non-default set (G3B_SET) runs over a slice of G3b (non-finite and huge logits).  Only outputs are stored; the inputs are
rebuilt by tests/m2p_params_cases.py.  The defaults must reproduce G3 and G9 where eli_structual_error leaves the QT map alone.
"""
import os
import sys
import warnings
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import m2p_params_cases as K

OUT = os.path.join(ROOT, "tests", "golden", "g10_m2p_params.npz")
_REF = None


def _ref():
    global _REF
    if _REF is None:
        import ref_harness as R
        _REF = R.load()
    return _REF


def eli(qt):
    import torch
    _, Met, _, _ = _ref()
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        return Met.eli_structual_error(torch.from_numpy(np.ascontiguousarray(qt, np.float32)[:, None].copy())).numpy()[:, 0]


def run(job):
    """job = (set name, source, cf, fixed qt, bt, dire) -> (set name, source, cf, hor, ver, dout)"""
    name, src, cf, fixed, bt, dire = job
    _, _, M2P, _ = _ref()
    l1, l2, l3, l4, l5, thd = K.SETS[name]
    n = len(fixed)
    hor = np.zeros((n, 16, 16), np.uint8); ver = np.zeros((n, 16, 16), np.uint8); dout = np.zeros((n, 3, 16, 16), np.int8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(n):
            m = M2P.Map_to_Partition(fixed[i], bt[i], dire[i], cf, l1, l2, l3, l4, l5)
            m.msdire_map = M2P.th_round(dire[i], thd=thd)
            p, d = m.get_partition()
            hor[i], ver[i], dout[i] = p[0][:16, :16], p[1][:16, :16], d
    return name, src, cf, hor, ver, dout


def main():
    jobs = []
    for cf in (1, 2):
        for name in K.SETS:
            for src, qt, bt, dire in K.inputs(cf, K.SETS[name][5]):
                fixed = eli(qt)
                # split the large-tree slices so that the pool stays busy
                step = 1 if src == "g3t" else 64
                for o in range(0, len(qt), step):
                    jobs.append((name, "%s@%d" % (src, o), cf, fixed[o:o + step], bt[o:o + step], dire[o:o + step]))
        qt, bt, dire, fixed_ref = K.g3b_inputs(cf)
        fixed = eli(qt)
        assert np.array_equal(fixed, fixed_ref, equal_nan=True), "eli_structual_error differs from G3b's"
        jobs.append((K.G3B_SET, "g3b@0", cf, fixed, bt, dire))
    print("%d jobs" % len(jobs), flush=True)
    parts = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, tag, cf, h, v, d in pool.imap_unordered(run, jobs):
            src, off = tag.split("@")
            parts.setdefault((name, src, cf), []).append((int(off), h, v, d))
    out = {"meta": np.array("reference AolinFeng/PMP-VVC-TIP2023 Map2Partition.Map_to_Partition(lamb1..lamb5) + th_round(thd), numpy %s; "
                            "inputs: tests/m2p_params_cases.py" % np.__version__),
           "set_names": np.array(list(K.SETS)), "set_values": np.array([K.SETS[k] for k in K.SETS], np.float64)}
    for (name, src, cf), lst in parts.items():
        lst.sort(key=lambda t: t[0])
        for j, k in enumerate(("hor", "ver", "dout")):
            out["%s_%s_%s_cf%d" % (name, src, k, cf)] = np.concatenate([t[j + 1] for t in lst])
    # the defaults reproduce G3 / G9 where eli_structual_error is the identity on the fixture's QT map
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "g3_m2p.npz"))
    g9 = np.load(os.path.join(ROOT, "tests", "golden", "g9_m2p_seeded.npz"))
    for cf in (1, 2):
        for src, qt, _, _ in K.inputs(cf, 0.5):
            if src == "probe":
                continue
            same = np.all(eli(qt) == qt, axis=(1, 2))
            if src.startswith("g3"):
                t = src[2:]
                sl = dict(K.G3_SLICES)[t]
                ref = [g3["%s_%s_cf%d" % (t, k, cf)][sl] for k in ("hor", "ver", "dout")]
            elif src == "g9rand":
                ref = [g9["rand_%s_cf%d" % (k, cf)][dict(K.G9_SLICES)["rand"]] for k in ("hor", "ver", "dout")]
            else:                                 # g9raw: raw logits, the reference ran eli itself
                same[:] = True
                ref = [g9["raw_%s_cf%d" % (k, cf)][dict(K.G9_SLICES)["raw"]] for k in ("hor", "ver", "dout")]
            got = K.expected(out, "defaults", src, cf)
            for a, b in zip(got, ref):
                assert np.array_equal(a[same], b[same]), ("defaults differ from the older fixture", src, cf)
            print("defaults == older fixture: %s cf%d, %d of %d triples" % (src, cf, int(same.sum()), len(same)))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    for name in K.SETS:
        diff = sum(int(np.any(out["%s_%s_hor_cf%d" % (name, s, cf)] != out["defaults_%s_hor_cf%d" % (s, cf)], axis=(1, 2)).sum())
                   for cf in (1, 2) for s, _, _, _ in K.inputs(cf, 0.5) if s != "probe")
        print("%-11s %s: %d non-probe triples with edges other than the defaults'" % (name, K.SETS[name], diff))


if __name__ == "__main__":
    main()
