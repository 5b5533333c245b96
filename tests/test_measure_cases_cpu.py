"""GPU-free guards of the evaluation-kernel tests (tests/measure_cases.py):

  * the tile sizes are read from tf2_yolo_amd/csrc/measure.hip and every case of the table is checked against them -- a later
    change of a tile must not turn the "past one tile" tests back into one-tile tests unnoticed;
  * the references are checked against what they restate: ref_rank_desc against np.argsort(key)[::-1] where that is defined
    (no ties, no NaN), ref_pr_curve against oracle.measurement.pr_curves on the golden fixture;
  * the decision margin of every match case and end-to-end fixture: no reference IoU lies within 1e-9 of the threshold and no
    two candidate ground truths of a detection lie that close to each other. The kernel may contract
    `b2*b3 + a2*a3 - inter` into fused multiply-adds, so its IoU can differ from NumPy's in the last bits (about 1e-16
    absolute); with the margin, a disagreement about a decision is a fault of the kernel, not a coin-flip of the inputs."""
import os
import re

import numpy as np
import pytest

import measure_cases as MC
from measure_cases import OM, gen_inputs
from make_measurement_golden import PR_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    with open(os.path.join(ROOT, "tf2_yolo_amd", "csrc", "measure.hip")) as f:
        return f.read()


def _kernel(src, name):
    m = re.search(r"__global__[^;{]*\b%s\((.*?)\n}\n" % name, src, re.S)
    assert m, f"{name} not found in measure.hip: revisit tests/measure_cases.py"
    return m.group(1)


def test_tiles_in_the_source_are_the_tiles_of_the_table():
    src = _src()
    rank = _kernel(src, "rank_desc_images_kernel")
    assert set(re.findall(r"base \+= (\d+)", rank)) == {str(MC.RANK_TILE)}
    lds = dict(re.findall(r"__shared__ \w+ (s_\w+)\[(\d+)\]", rank))
    assert lds == {"s_key": str(MC.RANK_TILE), "s_cls": str(MC.RANK_TILE), "s_range": "2"}, lds      # two tiles and one range
    assert re.search(r"w0 = blockIdx\.x \* %d;" % MC.RANK_TILE, rank) and "i = w0 + threadIdx.x;" in rank
    assert re.search(r"__launch_bounds__\(%d\) void rank_desc_images_kernel" % MC.RANK_TILE, src)
    scan = _kernel(src, "prc_scan_kernel")
    assert set(re.findall(r"base \+= (\d+)", scan)) == {str(MC.SCAN_CHUNK)}
    assert re.search(r"__launch_bounds__\(%d\) void prc_scan_kernel" % MC.SCAN_CHUNK, src)
    assert re.findall(r"__shared__ int s_w\[(\d+)\]", scan) == [str(MC.SCAN_CHUNK // 64)]            # one count per wave
    # every launch of the file is written so that this pattern reads it: one that it cannot read is a failure, not a skip
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\((.*?)\), dim3\((\d+)\), 0,", src)
    assert len(launches) == src.count("hipLaunchKernelGGL") == 16, launches
    kernels = set(re.findall(r"__global__[^;{]*?void (\w+)\(", src))
    assert len(kernels) == 12 and {name for name, _, _ in launches} == kernels, (kernels, launches)
    per_class = {"prc_scan_kernel": MC.SCAN_CHUNK,          # one workgroup per class: the chunk carry stays in registers
                 "prc_partition_kernel": MC.SCAN_CHUNK}     # one workgroup per class: the same 16-wave prefix count
    for name, grid, block in launches:
        if name in per_class:
            assert grid in ("C", "class_num") and int(block) == per_class[name], (name, grid, block)
        elif name == "prc_offsets_kernel":                  # one thread scans the class counts: C is small
            assert (grid, int(block)) == ("1", 64)
        else:
            assert int(block) == MC.LAUNCH_BLOCK, (name, grid, block)
            assert re.fullmatch(r"(?:\(unsigned\)\()?\(\w+ \+ %d\) / %d\)?" % (int(block) - 1, int(block)), grid), (name, grid)


def test_kernel_cases_sit_on_the_tile_edges_and_past_them():
    t = MC.RANK_TILE
    assert {t - 1, t, t + 1} <= set(MC.RANK_NS) and max(MC.RANK_NS) > 3 * t and 1 in MC.RANK_NS
    dets, gts = {c.ndet for c in MC.MATCH_CASES}, {c.ngt for c in MC.MATCH_CASES}
    b = MC.LAUNCH_BLOCK
    assert {0, 1, b - 1, b, b + 1} <= dets and {0, 1} <= gts
    big = MC.MATCH_BY_NAME["gt300-det700"]
    assert big.ngt > b and big.ndet > 2 * b       # a second workgroup over the ground truths, a third over the detections
    s = MC.SCAN_CHUNK
    assert {1, s - 1, s, s + 1} <= set(MC.PR_NS)
    assert sum(2 * s < n <= 3 * s for n in MC.PR_NS) >= 1 and max(MC.PR_NS) > 3 * s
    assert all(n % s for n in MC.PR_NS if n > s + 1)      # the last chunk is partial


@pytest.mark.parametrize("segmented", [False, True])
@pytest.mark.parametrize("n", MC.RANK_NS)
def test_rank_cases_hold_what_they_promise(n, segmented):
    for kind in MC.RANK_KINDS:
        key, seg = MC.rank_case(n, segmented, kind)
        assert key.dtype == np.float64 and key.shape == (n,) and (seg is None) == (not segmented)
        if segmented and n >= 255:
            sizes = np.bincount(seg, minlength=MC.RANK_SEGMENTS)
            assert len(sizes) == MC.RANK_SEGMENTS and sizes[-1] == 1 and len(set(sizes)) == MC.RANK_SEGMENTS
            assert (np.diff(seg) != 0).sum() > n // 2                   # interleaved
        if n >= 255:
            if kind == "five" and n >= 2 * MC.RANK_TILE:
                assert len(np.unique(key)) == 5
                runs = [np.flatnonzero(key == v) for v in np.unique(key)]
                assert all(r[0] < MC.RANK_TILE <= r[-1] for r in runs)   # every tie run crosses the first tile edge
            if kind == "special":
                assert (np.signbit(key) & (key == 0)).sum() > 5 and (~np.signbit(key) & (key == 0)).sum() > 5
                assert (key == np.inf).sum() > 5 and (key == -np.inf).sum() > 5
            if kind == "nan1":
                per = np.bincount(seg[np.isnan(key)], minlength=MC.RANK_SEGMENTS) if segmented else [np.isnan(key).sum()]
                assert all(p == 1 for p in per)
            if kind == "nan3":
                assert 0.25 < np.isnan(key).mean() < 0.42
        rank = MC.ref_rank_desc(key, seg)
        for s in (np.unique(seg) if segmented else [0]):
            rows = rank[seg == s] if segmented else rank
            assert np.array_equal(np.sort(rows), np.arange(len(rows)))


@pytest.mark.parametrize("n", [1, 2, 257, 1000])
def test_ref_rank_desc_is_argsort_reversed_without_ties(n):
    key = np.random.default_rng(n).normal(size=n)
    key[: n // 3] = np.arange(n // 3)                  # and some integers, -0.0 not among them
    assert len(np.unique(key)) == n
    order = np.argsort(key)[::-1]
    assert np.array_equal(MC.ref_order(key), order)
    rank = MC.ref_rank_desc(key)
    assert np.array_equal(rank[order], np.arange(n))
    seg = (np.arange(n) * 7 % 3).astype(np.int32)
    rank = MC.ref_rank_desc(key, seg)
    for s in range(3):
        rows = np.flatnonzero(seg == s)
        assert np.array_equal(rank[rows[np.argsort(key[rows])[::-1]]], np.arange(len(rows)))


def test_ref_rank_desc_order_rule():
    nan, inf = np.nan, np.inf
    #                0     1    2    3    4     5    6     7
    key = np.array([0.5, nan, 0.0, inf, -0.0, nan, 0.5, -inf])
    # NaN orders as +inf and equal keys put the higher index first: 5 (NaN), 3 (inf), 1 (NaN), 6, 0, 4 (-0.0), 2 (0.0), 7
    assert list(MC.ref_order(key)) == [5, 3, 1, 6, 0, 4, 2, 7]
    assert list(MC.ref_rank_desc(key)) == [4, 2, 6, 1, 5, 0, 3, 7]


@pytest.mark.parametrize("key,kw", PR_CASES)
def test_ref_pr_curve_matches_the_oracle_on_the_golden_fixture(key, kw):
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    ps, rs = OM.pr_curves(y_true, (lv0, lv1), 3, version=3, **kw)
    rec_kw = {k: v for k, v in kw.items() if k != "precision_mode"}
    recs, gts = OM.class_records(y_true, (lv0, lv1), 3, version=3, **rec_kw)
    for c in range(3):
        assert len(np.unique(recs[c][:, 0])) == len(recs[c])             # the fixture has no ties
        p, r = MC.ref_pr_curve(recs[c][:, 0], recs[c][:, 1], recs[c][:, 2], gts[c], kw["precision_mode"])
        assert np.array_equal(p, ps[c]) and np.array_equal(r, rs[c]), (key, c)


@pytest.mark.parametrize("case", MC.MATCH_CASES, ids=lambda c: c.name)
def test_match_case_holds_what_it_promises(case):
    gt, det = MC.match_case(case.name)
    assert gt.shape == (case.ngt, 7) and det.shape == (case.ndet, 7)
    best_gt, matched, best_iou, counts = MC.match_reference(case.name)
    gcls, dcls = gt[:, 5].astype(int), det[:, 5].astype(int)
    m_thr, m_arg = MC.decision_margins(gt, det, case.thr)
    print(f"MEASURE_MARGIN {case.name}: |IoU - {case.thr}| >= {m_thr:.3g}, best - next IoU >= {m_arg:.3g}")
    assert m_thr > MC.MARGIN and m_arg > MC.MARGIN
    assert counts[:, 0].sum() == ((dcls >= 0) & (dcls < 3)).sum() and counts[:, 1].sum() == ((gcls >= 0) & (gcls < 3)).sum()
    if case.flavour == "empty-class":
        assert counts[2, 0] > 20 and counts[2, 1] == 0 and not matched[dcls == 2].any()
    if case.flavour in ("duplicates", "everything"):
        first, later = (1, 4) if case.flavour == "duplicates" else (10, 200)
        assert np.array_equal(gt[first], gt[later])
        k_first = int((gcls[:first] == gcls[first]).sum())              # index inside the class subset
        k_later = int((gcls[:later] == gcls[first]).sum())
        on_it = (dcls == gcls[first]) & (best_gt == k_first) & (matched == 1)
        assert on_it.sum() >= 10 and not ((dcls == gcls[first]) & (best_gt == k_later)).any()
    if case.flavour == "disjoint":
        assert case.thr == 0.0 and (best_iou == 0.0).all() and (best_gt == 0).all()
        assert matched[dcls < 2].all() and not matched[dcls == 2].any()
        assert list(counts[:, 3]) == [1, 1, 0] and counts[0, 2] == counts[0, 0] > 1
    if case.flavour == "everything":
        assert {-1, 3} <= set(gcls) and {-1, 3} <= set(dcls)
        assert matched[dcls == -1].any() or matched[dcls == 3].any()    # matched among themselves, counted nowhere
    if case.ngt and case.ndet > 1:
        assert (counts[:, 3] < counts[:, 2]).any()                       # two detections on one ground truth: tp < tpp
        assert 0 < matched.sum() < case.ndet


def test_pr_cases_hold_what_they_promise():
    for n in MC.PR_NS:
        for g in MC.PR_NUM_GTS:
            joint, gid, matched = MC.pr_case(n, g, "mixed")
            assert gid.min() >= 0 and gid.max() < g and len(np.unique(joint)) == n
            if n > 1000:
                assert 0.45 < matched.mean() < 0.55
                if g <= 300:
                    assert np.bincount(gid[matched == 1]).max() > 1    # several matched detections per ground truth
    joint, gid, matched = MC.pr_case(3100, 300, "ties")
    assert len(np.unique(joint)) == 5
    for m in (0, 2):   # the tie rule decides the curve: the other order of the tied rows gives another one
        p, r = MC.pr_reference(3100, 300, "ties", m)
        rec = np.stack((joint, gid.astype(np.float64), matched.astype(np.float64)), axis=1)
        p2, r2 = OM.curve_from_records(rec, 300, m, order=np.argsort(-joint, kind="stable"))
        assert not np.array_equal(p, p2)
    joint, _, _ = MC.pr_case(3100, 300, "nan")
    assert np.isnan(joint).sum() > 400 and (joint == np.inf).sum() == 3
    assert not MC.pr_case(2500, 300, "none")[2].any() and MC.pr_case(2500, 300, "all")[2].all()
    p, r = MC.pr_reference(1, 1, "nan", 2)
    assert np.isnan(MC.pr_case(1, 1, "nan")[0][0]) and np.isfinite(p).all() and np.isfinite(r).all()


@pytest.fixture(scope="module")
def many_rows():
    y_true, lv0, lv1 = MC.many_inputs()
    return MC.image_rows(y_true, (lv0, lv1), MC.MANY_CLASSES)


def test_many_images_fixture_lies_past_two_scan_chunks(many_rows):
    _, _, per_class = MC.size_stats(many_rows, MC.MANY_CLASSES)
    gts = np.sum([np.bincount(g[:, 5].astype(int), minlength=2) for g, _ in many_rows], axis=0)
    print(f"MEASURE_SIZES many: detections per class {list(per_class)}, ground truths per class {list(gts)}")
    assert (per_class > 2 * MC.SCAN_CHUNK).all() and (per_class % MC.SCAN_CHUNK != 0).all()
    m = [MC.decision_margins(g, d, 0.5) for g, d in many_rows]
    print(f"MEASURE_MARGIN many: |IoU - 0.5| >= {min(a for a, _ in m):.3g}, best - next IoU >= {min(b for _, b in m):.3g}")
    assert min(a for a, _ in m) > MC.MARGIN and min(b for _, b in m) > MC.MARGIN


def test_tied_fixture_has_ties_where_the_cut_and_the_curve_decide():
    y_true, lv0, lv1 = MC.tied_inputs()
    rows = MC.image_rows(y_true, (lv0, lv1), MC.MANY_CLASSES)
    cut = MC.TIES_KW["max_per_img"]
    straddle = 0          # (image, class) sets whose cut falls inside a run of equal joint confidences
    for _, det in rows:
        for c in range(MC.MANY_CLASSES):
            j = np.sort((det[:, 4] * det[:, 6])[det[:, 5].astype(int) == c])[::-1]
            straddle += len(j) > cut and j[cut - 1] == j[cut]
    recs, _ = OM.class_records(y_true, (lv0, lv1), MC.MANY_CLASSES, order=MC.ref_order, **MC.TIES_KW)
    mixed = 0             # runs of equal joint confidences on the curve that hold matched and unmatched rows
    for rec in recs:
        assert len(rec) > MC.SCAN_CHUNK
        for v in np.unique(rec[:, 0]):
            hits = rec[rec[:, 0] == v, 2]
            mixed += 0 < hits.sum() < len(hits)
    print(f"MEASURE_TIES: the cut splits a tie run in {straddle} (image, class) sets; {mixed} tie runs of the curves are mixed")
    assert straddle >= 10 and mixed >= 10
    m = [MC.decision_margins(g, d, 0.5) for g, d in rows]
    assert min(a for a, _ in m) > MC.MARGIN and min(b for _, b in m) > MC.MARGIN
    # and the order matters: the reference's unstable argsort gives other curves on this input
    ps, _ = OM.pr_curves(y_true, (lv0, lv1), MC.MANY_CLASSES, order=MC.ref_order, **MC.TIES_KW)
    ps2, _ = OM.pr_curves(y_true, (lv0, lv1), MC.MANY_CLASSES, order=lambda k: np.argsort(-k, kind="stable"), **MC.TIES_KW)
    assert any(not np.array_equal(a, b) for a, b in zip(ps, ps2))


def test_dense_fixture_lies_past_the_launch_and_count_tiles():
    """more than one 256-thread workgroup over the detections (mb_match_kernel) and over the ground truths, which
    mb_distinct_kernel counts, of ONE image"""
    y_true, lv0, lv1 = MC.dense_inputs()
    rows = MC.image_rows(y_true, (lv0, lv1), MC.DENSE_CLASSES, **MC.DENSE_KW)
    per_image = [len(d) for _, d in rows]
    print(f"MEASURE_SIZES dense: detections per image {per_image}, ground truths per image {[len(g) for g, _ in rows]}")
    assert min(per_image) > 2 * MC.LAUNCH_BLOCK and all(len(g) == 400 > MC.LAUNCH_BLOCK for g, _ in rows)
    for _, det in rows:       # the cap of 100 per image and class really cuts
        assert (np.bincount(det[:, 5].astype(int), minlength=3) > 2 * MC.DENSE_KW["max_per_img"]).all()
    for thr in MC.DENSE_THRESHOLDS:
        m = [MC.decision_margins(g, d, thr) for g, d in rows]
        print(f"MEASURE_MARGIN dense: |IoU - {thr}| >= {min(a for a, _ in m):.3g}, best - next IoU >= {min(b for _, b in m):.3g}")
        assert min(a for a, _ in m) > MC.MARGIN and min(b for _, b in m) > MC.MARGIN
        ps, _ = OM.pr_curves(y_true, (lv0, lv1), MC.DENSE_CLASSES, iou_threshold=thr, **MC.DENSE_KW)
        assert [len(p) for p in ps] == [2 * MC.DENSE_KW["max_per_img"] + 1] * 3
