"""The evaluation kernels (tf2_yolo_amd/csrc/measure.hip) through ops, one by one, against the float64 NumPy references of
tests/measure_cases.py: at the tile edges (255 / 256 / 257 rows, 1023 / 1024 / 1025 sorted flags), past them (several rank
tiles, a second workgroup of every grid, the strided loops of the count kernel, the chunk carry of the scan), with score
ties, NaN scores and class ids outside the range. tests/test_measure_cases_cpu.py guards the table without a GPU."""
import numpy as np
import pytest
import torch

import measure_cases as MC

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the cases are read-only)


# ---- ops.rank_desc --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MC.RANK_KINDS)
@pytest.mark.parametrize("segmented", [False, True], ids=["one-segment", "seven-segments"])
@pytest.mark.parametrize("n", MC.RANK_NS)
def test_rank_desc(n, segmented, kind):
    """ranks bit-equal to ref_rank_desc: keys descending, NaN as +inf, equal keys the higher index first"""
    from tf2_yolo_amd import ops
    key, seg = MC.rank_case(n, segmented, kind)
    got = ops.rank_desc(_dev(key), _dev(seg)).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (n,)
    for s in (np.unique(seg) if segmented else [0]):        # a permutation of 0 .. m-1 inside every segment
        rows = got[seg == s] if segmented else got
        assert np.array_equal(np.sort(rows), np.arange(len(rows))), (s, np.bincount(rows.clip(0)).max())
    assert np.array_equal(got, MC.ref_rank_desc(key, seg))


def test_rank_desc_of_nothing():
    from tf2_yolo_amd import ops
    assert ops.rank_desc(torch.empty(0, dtype=torch.float64, device="cuda")).shape == (0,)


# ---- ops.match_detections -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.MATCH_CASES, ids=lambda c: c.name)
def test_match_detections(case):
    """best_gt and matched equal the reference, best_iou within 1e-12 relative (the kernel may contract
    `b2*b3 + a2*a3 - inter` into fused multiply-adds: a few ulp, about 1e-15); the counts exactly, accumulated over two
    calls into the same class_counts"""
    from tf2_yolo_amd import ops
    gt, det = MC.match_case(case.name)
    best_gt, matched, best_iou, counts = MC.match_reference(case.name)
    acc = torch.zeros((MC.MATCH_CLASSES, 4), device="cuda", dtype=torch.int64)
    for call in (1, 2):
        g_best, g_matched, g_iou = ops.match_detections(_dev(gt), _dev(det), MC.MATCH_CLASSES, case.thr, acc)
        assert g_best.dtype == torch.int32 and g_matched.dtype == torch.uint8 and g_iou.dtype == torch.float64
        assert np.array_equal(g_best.cpu().numpy(), best_gt), call
        assert np.array_equal(g_matched.cpu().numpy(), matched), call
        g_iou = g_iou.cpu().numpy()
        err = np.abs(g_iou - best_iou)
        worst = float((err / np.maximum(np.abs(best_iou), 1e-300)).max()) if case.ndet else 0.0
        print(f"MEASURE_IOU {case.name}: worst relative best_iou difference {worst:.3g} (bound 1e-12)")
        assert g_iou.shape == best_iou.shape and (err <= 1e-12 * np.abs(best_iou)).all(), worst
        assert np.array_equal(acc.cpu().numpy(), call * counts), call


# ---- ops.pr_curve ---------------------------------------------------------------------------------------------------
def _pr(n, num_gts, kind, mode, poison=False):
    from tf2_yolo_amd import _lib, ops
    joint, gid, matched = MC.pr_case(n, num_gts, kind)
    args = (_dev(joint), _dev(gid), _dev(matched))
    if poison:      # the workspace comes from torch.empty: hand the caching allocator a block of its size full of 0xFF
        nbytes = int(_lib.load().yolo_pr_curve_workspace_bytes(n, num_gts))
        block = torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)
        del block
    p, r = ops.pr_curve(*args, num_gts, mode)
    want_p, want_r = MC.pr_reference(n, num_gts, kind, mode)
    p, r = p.cpu().numpy(), r.cpu().numpy()
    assert p.shape == r.shape == (n + 1,)
    assert np.isfinite(p).all() and np.isfinite(r).all()
    bad = np.flatnonzero((p != want_p) | (r != want_r))
    assert bad.size == 0, (bad[:5], p[bad[:5]], want_p[bad[:5]], r[bad[:5]], want_r[bad[:5]])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("num_gts", MC.PR_NUM_GTS)
@pytest.mark.parametrize("n", MC.PR_NS)
def test_pr_curve(n, num_gts, mode):
    """precision and recall bit-equal to ref_pr_curve (one division of two integers each): about half of the rows matched,
    several matched rows per ground-truth id wherever n / 2 > num_gts"""
    _pr(n, num_gts, "mixed", mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["none", "all"])
def test_pr_curve_no_row_or_every_row_matched(kind, mode):
    _pr(2500, 300, kind, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [257, 1025, 3100])
def test_pr_curve_tied_scores(n, mode):
    """five distinct scores: the tied rows differ in `matched`, so the tie rule (the higher index first) decides the curve"""
    _pr(n, 300, "ties", mode)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n,num_gts", [(1, 1), (255, 300), (1023, 1), (1025, 300), (3100, 300)])
def test_pr_curve_nan_scores(n, num_gts, mode):
    """NaN scores order as +inf. Without a total order the ranks are no permutation and slots of the sorted flags stay
    unwritten: the workspace's memory is filled with 0xFF beforehand so that such a slot shows"""
    _pr(n, num_gts, "nan", mode, poison=True)


def test_pr_curve_rejections():
    from tf2_yolo_amd import _lib, ops
    from tf2_yolo_amd._lib import YoloHipError
    joint, gid, matched = (_dev(a) for a in MC.pr_case(255, 300, "mixed"))
    with pytest.raises(YoloHipError):
        ops.pr_curve(joint[:0], gid[:0], matched[:0], 300, 2)
    with pytest.raises(YoloHipError):
        ops.pr_curve(joint, gid, matched, 0, 2)
    with pytest.raises(YoloHipError):
        ops.pr_curve(joint, gid, matched, 300, 3)
    with pytest.raises(YoloHipError):
        ops.pr_curve(joint, gid, matched, 300, -1)
    lib = _lib.load()
    nbytes = int(lib.yolo_pr_curve_workspace_bytes(255, 300))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    out = torch.full((2, 256), -7.0, device="cuda", dtype=torch.float64)
    args = (ops._p(joint), ops._p(gid), ops._p(matched), 255, 300, 2, ops._p(ws))
    assert lib.yolo_pr_curve(*args, nbytes - 1, ops._p(out[0]), ops._p(out[1]), ops._stream()) != 0
    assert b"workspace too small" in lib.yolo_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()                      # a rejected call launches nothing
    assert lib.yolo_pr_curve(*args, nbytes, ops._p(out[0]), ops._p(out[1]), ops._stream()) == 0
    want_p, want_r = MC.pr_reference(255, 300, "mixed", 2)
    assert np.array_equal(out[0].cpu().numpy(), want_p) and np.array_equal(out[1].cpu().numpy(), want_r)
