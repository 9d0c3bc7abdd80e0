"""CPU: the numpy restatement of the confusion rule (tests/confusion_cases.py) is pinned against torch.round and hand-written cells, and
engine.confusion_summary against counts whose parts are known."""
import numpy as np
import pytest

import confusion_cases as X


@pytest.mark.parametrize("n,seed", [(1, 1), (3, 2), (17, 3)])
def test_diagonal_is_the_references_hit_count(n, seed):
    import torch
    c = X.in_range(n, seed)
    C = X.counts(**c)
    ql = torch.from_numpy((c["qt8"] - np.uint8(1)).astype(np.float32))
    want = [int(torch.sum(torch.round(torch.from_numpy(c["qt"])) == ql))]
    want += [int(torch.sum(torch.round(torch.from_numpy(c["bt"][:, k])) == torch.from_numpy(c["msbt"][:, k].astype(np.float32)))) for k in range(3)]
    want += [int(torch.sum(torch.round(torch.from_numpy(c["dire"][:, k])) == torch.from_numpy(c["msdire"][:, k].astype(np.float32)))) for k in range(3)]
    assert X.diagonal(C).tolist() == want
    assert C[0].sum() == 64 * n and all(C[m].sum() == 256 * n for m in range(1, 7))
    assert not C[4:, 4, :].any() and not C[4:, :, 4].any()           # class 4 stays zero on the direction maps
    assert X.block_counts(**c).max() <= 256


def test_hand_written_logits():
    want = {0.5: (0, 1), 1.5: (2, 3), 2.5: (2, 3), 3.5: (4, 3), -0.4: (0, 1), -0.5: (0, 1), -0.51: (4, 0), 1e30: (4, 3)}
    for x, (d, r) in want.items():
        assert X.depth_class(X.predicted([x]))[0] == d, x
        assert X.dire_class(X.predicted([x]))[0] == r, x
    for x in (float("nan"), float("inf"), -float("inf")):
        assert X.depth_class(X.predicted([x]))[0] == 4 and X.dire_class(X.predicted([x]))[0] == 3
    for x, d, r in X.SPECIAL_LOGITS:                                  # the table the GPU test plants says the same
        assert (X.depth_class(X.predicted([x]))[0], X.dire_class(X.predicted([x]))[0]) == (d, r), x


def test_hand_written_labels():
    one = lambda raw: X.counts(qt=np.zeros((1, 8, 8), np.float32), qt8=np.full((1, 8, 8), raw, np.uint8))[0]
    assert one(0)[4, 0] == 64                                         # raw 0 -> label 255: other
    assert one(5)[4, 0] == 64                                         # raw 5 -> label 4: other
    assert one(1)[0, 0] == 64 and one(4)[3, 0] == 64
    for raw, cls in X.SPECIAL_QT8:
        assert one(raw)[cls].sum() == 64
    z = np.zeros((1, 3, 16, 16), np.float32)

    def mtt(b, d):
        return X.counts(bt=z, dire=z, msbt=np.full(z.shape, b, np.uint8), msdire=np.full(z.shape, d, np.int8))
    assert mtt(4, 0)[1, 4, 0] == 256 and mtt(200, 0)[2, 4, 0] == 256
    assert mtt(0, 2)[4, 3, 1] == 256 and mtt(0, -128)[6, 3, 1] == 256
    for raw, cls in X.SPECIAL_MSBT:
        assert mtt(raw, 0)[1, cls, 0] == 256
    for raw, cls in X.SPECIAL_MSDIRE:
        assert mtt(0, raw)[4, cls, 1] == 256


def test_census_and_forms():
    c = X.special(2)
    full = X.counts(**c)
    cen = X.counts(**X.form(c, "census"))
    assert np.array_equal(cen.sum(axis=2), full.sum(axis=2))         # the row sums are the label counts
    assert cen[:4, :, :4].sum() == 0 and cen[4:, :, :3].sum() == 0 and cen[4:, :, 4].sum() == 0
    q = X.counts(**X.form(c, "q"))
    assert np.array_equal(q[0], full[0]) and not q[1:].any()
    m = X.counts(**X.form(c, "m"))
    assert np.array_equal(m[1:], full[1:]) and not m[0].any()
    mix = X.counts(**X.form(c, "q+census_m"))
    assert np.array_equal(mix[0], full[0]) and np.array_equal(mix[1:], cen[1:])


def test_summary_parts():
    from pmp_vvc_tip2023_amd import engine
    C = np.zeros((7, 5, 5), np.int64)
    C[0] = np.arange(25).reshape(5, 5)
    C[4, :4, :4] = np.arange(16).reshape(4, 4)
    s = engine.confusion_summary(C)
    q, tot = s["qt"], 300.0
    assert q["total"] == 300 and q["matrix"] == C[0].tolist()
    assert q["hit"] == (0 + 6 + 12 + 18) / tot
    assert q["under"] == (5 + 10 + 11 + 15 + 16 + 17) / tot and q["over"] == (1 + 2 + 3 + 7 + 8 + 13) / tot
    assert q["other_label"] == sum(range(20, 25)) / tot and q["other_pred"] == (4 + 9 + 14 + 19) / tot
    assert q["label_freq"] == [v / tot for v in C[0].sum(axis=1)]
    d, tot = s["dire0"], 120.0
    assert d["hit"] == (0 + 5 + 10) / tot and d["missed"] == (1 + 9) / tot and d["false"] == (4 + 6) / tot and d["flipped"] == (2 + 8) / tot
    assert d["other_label"] == (12 + 13 + 14 + 15) / tot and d["other_pred"] == (3 + 7 + 11) / tot
    assert s["bt1"]["total"] == 0 and s["bt1"]["hit"] == 0.0
    for m in s.values():
        parts = [k for k in m if k not in ("matrix", "total", "label_freq")]
        assert m["total"] == 0 or abs(sum(m[k] for k in parts) - 1.0) < 1e-12


def test_tool_flags_are_checked_before_the_gpu(tmp_path, capsys):
    from pmp_vvc_tip2023_amd import train_qbd, validate
    assert validate.build_parser().parse_args(["--dataDir", "d", "--comp", "Luma", "--qp", "22", "--confusion"]).confusion
    assert train_qbd.build_parser().parse_args(["--confusion"]).confusion and not train_qbd.build_parser().parse_args([]).confusion
    # --mode labels opens the label files alone: no block file is needed
    qt8 = np.ones((3, 8, 8), np.uint8)
    np.save(str(tmp_path / "Validate_Luma_QP22_QTdepth_Block8.npy"), qt8)
    args = validate.build_parser().parse_args(["--dataDir", str(tmp_path), "--comp", "Luma", "--qp", "22", "--mode", "labels"])
    d = validate.plan(args)
    assert d["n"] == 3 and d["blocks"] is None and d["msbt"] is None
    args = validate.build_parser().parse_args(["--dataDir", str(tmp_path), "--comp", "Luma", "--qp", "22", "--mode", "census"])
    with pytest.raises(SystemExit) as e:
        validate.plan(args)
    assert e.value.code == 2
