"""The evaluation kernels (tf2_yolo_amd/csrc/measure.hip) through the one-image / one-class front ends of ops, one by one,
against the float64 NumPy references of tests/measure_cases.py: at the tile edges (255 / 256 / 257 rows, 1023 / 1024 / 1025
sorted flags), past them (several rank tiles, a second workgroup of every grid over detections and ground truths, the
chunk carry of the scan), with score ties, NaN scores and class ids outside the range. tests/test_measure_cases_cpu.py guards the table without a GPU."""
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


@pytest.mark.parametrize("name", ["gt300-det700", "gt1-det1"])
def test_match_detections_zeroes_the_callers_flags(name):
    """gt_flags comes uninitialised: the raw call with the flags full of 0xFF, twice into the same class_counts, counts
    what the reference counts, and leaves one flag per distinct matched ground truth of a class in range"""
    from tf2_yolo_amd import _lib, ops
    case = MC.MATCH_BY_NAME[name]
    gt, det = (_dev(a) for a in MC.match_case(name))
    counts = MC.match_reference(name)[3]
    lib = _lib.load()
    acc = torch.zeros((MC.MATCH_CLASSES, 4), device="cuda", dtype=torch.int64)
    best_gt = torch.empty(case.ndet, device="cuda", dtype=torch.int32)
    matched = torch.empty(case.ndet, device="cuda", dtype=torch.uint8)
    best_iou = torch.empty(case.ndet, device="cuda", dtype=torch.float64)
    for call in (1, 2):
        flags = torch.full((case.ngt,), 0xFF, device="cuda", dtype=torch.uint8)
        assert lib.yolo_match_detections(ops._p(gt), case.ngt, ops._p(det), case.ndet, MC.MATCH_CLASSES, float(case.thr),
                                         ops._p(best_gt), ops._p(matched), ops._p(best_iou), ops._p(flags), ops._p(acc),
                                         ops._stream()) == 0
        assert np.array_equal(acc.cpu().numpy(), call * counts), call
        assert int(flags.max()) <= 1 and int(flags.sum()) == counts[:, 3].sum(), call


@pytest.mark.parametrize("name", ["gt300-det0", "gt0-det300"])
def test_match_detections_with_one_side_empty(name):
    """no detections: only the ground-truth column of the counts advances; no ground truths: only the detection column, and
    nothing is matched (both cases are rows of MC.MATCH_CASES, so test_match_detections holds them to the reference too)"""
    from tf2_yolo_amd import ops
    case = MC.MATCH_BY_NAME[name]
    gt, det = MC.match_case(name)
    acc = torch.zeros((MC.MATCH_CLASSES, 4), device="cuda", dtype=torch.int64)
    for call in (1, 2):
        _, g_matched, _ = ops.match_detections(_dev(gt), _dev(det), MC.MATCH_CLASSES, case.thr, acc)
        got = acc.cpu().numpy()
        side, rows = (1, gt) if case.ndet == 0 else (0, det)
        assert np.array_equal(got[:, side], call * np.bincount(rows[:, 5].astype(int), minlength=MC.MATCH_CLASSES)), call
        assert got[:, side].sum() == call * len(rows) and not np.delete(got, side, axis=1).any(), call
        assert g_matched.shape == (case.ndet,) and not g_matched.any()


def test_rank_desc_hostile_segment_ids():
    """segment ids are any ints, compared for equality only: negative ones, INT_MIN and INT_MAX, interleaved, one row past a
    tile, with a tie run across the tile edge and one NaN -- no id is a padding marker of the kernel"""
    from tf2_yolo_amd import ops
    n = MC.RANK_TILE + 1
    rng = np.random.default_rng(257)
    ids = np.array([-3, -2, -1, 0, 2**31 - 1, -2**31], dtype=np.int64)
    seg = ids[rng.permutation(np.arange(n) % len(ids))].astype(np.int32)
    key = rng.random(n)
    key[MC.RANK_TILE - 16:] = 0.5                              # rows 240 .. 256: a tie run of every segment across the edge
    key[7] = np.nan
    assert set(seg) == set(ids) and (np.diff(seg) != 0).sum() > n // 2
    assert (seg[MC.RANK_TILE - 16:MC.RANK_TILE] == seg[MC.RANK_TILE]).any()      # the last row ties with rows of the first tile
    got = ops.rank_desc(_dev(key), _dev(seg)).cpu().numpy()
    for s in ids:
        rows = got[seg == s]
        assert np.array_equal(np.sort(rows), np.arange(len(rows))), s
    assert np.array_equal(got, MC.ref_rank_desc(key, seg))


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


@pytest.mark.parametrize("n,num_gts", [(1, 1), (1025, 300)])
def test_pr_curve_is_pr_curves_of_a_one_class_data_set(n, num_gts):
    """the by-value class of yolo_pr_curve against the device tables of yolo_pr_curves: the same n + 1 points"""
    from tf2_yolo_amd import ops
    joint, gid, matched = (_dev(a) for a in MC.pr_case(n, num_gts, "mixed"))
    p, r = ops.pr_curve(joint, gid, matched, num_gts, 1)
    cls = torch.zeros(n, device="cuda", dtype=torch.int32)
    gts = torch.tensor([num_gts], device="cuda", dtype=torch.int64)
    cls_off, ps, rs = ops.pr_curves(joint, gid, matched, cls, gts, 1)
    assert cls_off.tolist() == [0, n] and p.shape == (n + 1,)
    assert torch.equal(ps, p) and torch.equal(rs, r)


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
