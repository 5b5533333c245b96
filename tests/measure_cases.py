"""Case tables and float64 NumPy references of the evaluation kernels (tf2_yolo_amd/csrc/measure.hip), GPU-free: nothing here
imports torch, the library or a device. tests/test_measure_cases_cpu.py checks the table against the tile sizes it reads
from the source; tests/test_gpu_measure_kernels.py and tests/test_gpu_measurement.py run the cases on the device.

The kernels work in tiles:

  rank tile    rank_desc_images_kernel walks the keys in tiles of 256; one workgroup covers 256 rows
  launch tile  mb_match_kernel over the detections, mb_distinct_kernel over the ground truths (and every other grid over
               rows of measure.hip) is a grid of 256-thread workgroups
  scan chunk   prc_scan_kernel walks the sorted flags in chunks of 1024 and carries a running (tpp, tp) pair

Size rule: the boundary cases sit at tile - 1, tile, tile + 1; a "past one tile" case has more than 256 detections and more
than 256 ground truths in one image (a second workgroup of both grids) and more than 2 x 1024 detections of one class (a
first, a middle and a last chunk).

The order (ref_rank_desc, ref_order): keys descend; the order key of NaN is +inf (np.argsort puts NaN last, so the
reference's argsort()[::-1] visits it first); equal order keys -- -0.0 and 0.0, two NaNs, NaN and +inf -- put the HIGHER
index first (np.argsort leaves ties to an unstable sort; the project defines them, as it does for NMS)."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_inputs                                    # noqa: E402

from oracle import measurement as OM                  # noqa: E402
from oracle import tools as OT                        # noqa: E402

RANK_TILE = 256          # rank_desc_images_kernel: rows per LDS tile and per workgroup
LAUNCH_BLOCK = 256       # threads per workgroup of every grid over rows (detections, ground truths, classes)
SCAN_CHUNK = 1024        # prc_scan_kernel: flags per chunk
MARGIN = 1e-9            # no reference IoU of a match case lies this close to the case's threshold


# ---- references ----------------------------------------------------------------------------------------------------
def ref_order(key):
    """visiting order (indices) of ONE segment: order key descending, equal order keys by index descending"""
    k = np.array(key, dtype=np.float64)
    k[np.isnan(k)] = np.inf
    return np.lexsort((-np.arange(len(k)), -k))     # the last key is the primary one; -(-0.0) == -(0.0) compares equal


def ref_rank_desc(key, segment=None):
    """yolo_rank_desc: rank[i] = number of rows of i's segment that are visited before row i"""
    key = np.asarray(key, dtype=np.float64)
    seg = np.zeros(len(key), dtype=np.int64) if segment is None else np.asarray(segment)
    rank = np.full(len(key), -1, dtype=np.int64)
    for s in np.unique(seg):
        rows = np.flatnonzero(seg == s)
        rank[rows[ref_order(key[rows])]] = np.arange(len(rows))
    return rank


def ref_match(gt_rows, det_rows, class_num, thr):
    """yolo_match_detections of one image -> (best_gt, matched, best_iou, counts [class_num, 4]).
    Class by class with oracle.measurement._match (oracle.tools.cal_iou, np.argmax: the first maximum); a detection
    whose class has no ground truth gets 0 / 0 / 0. The per-detection outputs are defined for EVERY detection by the
    rows of its own class id, in range or not; the counts hold the classes of [0, class_num) only."""
    gt = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 7)
    det = np.asarray(det_rows, dtype=np.float64).reshape(-1, 7)
    gcls, dcls = gt[:, 5].astype("int"), det[:, 5].astype("int")
    best_gt = np.zeros(len(det), dtype=np.int64)
    matched = np.zeros(len(det), dtype=np.uint8)
    best_iou = np.zeros(len(det), dtype=np.float64)
    counts = np.zeros((class_num, 4), dtype=np.int64)
    for c in np.unique(dcls):
        g, rows = gt[gcls == c], np.flatnonzero(dcls == c)
        if len(g) == 0:
            continue
        arg, hit = OM._match(g, det[rows], thr)
        best_gt[rows], matched[rows] = arg, hit
        best_iou[rows] = OT.cal_iou(g[:, :5].reshape(-1, 1, 5), det[rows][:, :5].reshape(1, -1, 5)).max(axis=0)
    for c in range(class_num):
        rows = np.flatnonzero(dcls == c)
        hit = matched[rows].astype(bool)
        counts[c] = (len(rows), int((gcls == c).sum()), int(hit.sum()), len(set(best_gt[rows][hit])))
    return best_gt, matched, best_iou, counts


def ref_pr_curve(joint, gid, matched, num_gts, mode):
    """yolo_pr_curve: oracle.measurement.curve_from_records with the sort replaced by ref_order"""
    rec = np.stack((np.asarray(joint, dtype=np.float64), np.asarray(gid, dtype=np.float64),
                    np.asarray(matched, dtype=np.float64)), axis=1)
    return OM.curve_from_records(rec, int(num_gts), mode, order=ref_order(rec[:, 0]))


def class_ious(gt_rows, det_rows):
    """yields (class id, IoU matrix [ground truths of the class, detections of the class], the ground-truth rows)"""
    gt = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 7)
    det = np.asarray(det_rows, dtype=np.float64).reshape(-1, 7)
    gcls, dcls = gt[:, 5].astype("int"), det[:, 5].astype("int")
    for c in np.unique(dcls):
        g, d = gt[gcls == c], det[dcls == c]
        if len(g) and len(d):
            yield int(c), OT.cal_iou(g[:, :5].reshape(-1, 1, 5), d[:, :5].reshape(1, -1, 5)), g


def decision_margins(gt_rows, det_rows, thr):
    """(threshold margin, argmax margin) of one image: the smallest |IoU - thr| and the smallest gap between the best and
    the next DIFFERENT IoU of a detection. An IoU of exactly 0 is left out of the first: an empty intersection is
    fmax(negative, 0) = 0 on the device too, and 0 / (union + 1e-7) = 0 whatever the union's last bits are. Equal best
    IoUs are checked to be exact on the device as well: zeros, or ground-truth rows with bit-identical boxes."""
    m_thr, m_arg = np.inf, np.inf
    for _, iou, g in class_ious(gt_rows, det_rows):
        nz = iou[iou != 0.0]
        if nz.size:
            m_thr = min(m_thr, float(np.abs(nz - thr).min()))
        top = iou.max(axis=0)
        for d in range(iou.shape[1]):
            lower = iou[:, d][iou[:, d] < top[d]]
            if lower.size:
                m_arg = min(m_arg, float(top[d] - lower.max()))
            tied = np.flatnonzero(iou[:, d] == top[d])
            assert top[d] == 0.0 or all(np.array_equal(g[t, :4], g[tied[0], :4]) for t in tied), "an accidental tie"
    return m_thr, m_arg


# ---- ops.rank_desc --------------------------------------------------------------------------------------------------
RANK_NS = [1, 255, 256, 257, 1000]
RANK_KINDS = ["continuous", "five", "special", "nan1", "nan3"]
RANK_SEGMENTS = 7


def rank_case(n, segmented, kind):
    """(key float64 [n], segment int32 [n] or None). Segments: seven interleaved ones of unequal size, the last of a
    single row (fewer of them where n is too small to hold all seven)."""
    rng = np.random.default_rng(1000 * n + 10 * RANK_KINDS.index(kind) + int(segmented))
    seg = None
    if segmented:
        sizes = np.floor(np.array([0.34, 0.25, 0.19, 0.11, 0.07, 0.04]) * (n - 1)).astype(int)
        sizes[0] += n - 1 - sizes.sum()
        seg = rng.permutation(np.repeat(np.arange(RANK_SEGMENTS), list(sizes) + [1])).astype(np.int32)
    if kind == "five":         # long tie runs that cross tile boundaries
        key = rng.choice(np.array([0.125, 0.3, 0.5, 0.7, 0.9]), size=n)
    else:
        key = rng.random(n)
    if kind == "special":      # -0.0 / 0.0 and +-inf, each many times
        sel = rng.random(n) < 0.5
        key[sel] = rng.choice(np.array([-0.0, 0.0, np.inf, -np.inf, 0.25]), size=int(sel.sum()))
    elif kind == "nan1":       # one NaN per segment
        for s in (np.unique(seg) if segmented else [0]):
            rows = np.flatnonzero(seg == s) if segmented else np.arange(n)
            key[rng.choice(rows)] = np.nan
    elif kind == "nan3":       # a third of the rows, and some +inf that tie with them
        key[rng.random(n) < 1 / 3] = np.nan
        key[rng.random(n) < 0.05] = np.inf
    return key, seg


# ---- ops.match_detections -------------------------------------------------------------------------------------------
MATCH_CLASSES = 3
MatchCase = namedtuple("MatchCase", "name ngt ndet thr seed flavour")
MATCH_CASES = [
    MatchCase("gt0-det300", 0, 300, 0.5, 1, "plain"),
    MatchCase("gt300-det0", 300, 0, 0.5, 2, "plain"),
    MatchCase("gt1-det1", 1, 1, 0.5, 3, "plain"),
    MatchCase("gt7-det255", 7, 255, 0.5, 4, "empty-class"),      # class 2 has detections and no ground truth
    MatchCase("gt7-det256", 7, 256, 0.5, 5, "duplicates"),       # duplicated ground-truth rows: exact IoU ties
    MatchCase("gt7-det257", 7, 257, 0.0, 6, "disjoint"),         # threshold 0.0, no box overlaps: IoU exactly 0, 0 >= 0
    MatchCase("gt300-det700", 300, 700, 0.5, 7, "everything"),   # + class ids -1 and class_num on both sides
]
MATCH_BY_NAME = {c.name: c for c in MATCH_CASES}


def _boxes(rng, n, lo=0.1, hi=0.9):
    rows = np.zeros((n, 7))
    rows[:, :2] = rng.random((n, 2)) * (hi - lo) + lo
    rows[:, 2:4] = rng.random((n, 2)) * 0.25 + 0.05
    rows[:, 4] = rng.random(n) * 0.9 + 0.1
    rows[:, 5] = rng.integers(0, MATCH_CLASSES, n)
    rows[:, 6] = rng.random(n) * 0.9 + 0.1
    return rows


@functools.lru_cache(maxsize=None)
def match_case(name):
    """(gt_rows [ngt,7], det_rows [ndet,7]) float64, read-only. Detections: two thirds noisy copies of a ground truth
    (four fifths of them with its class), one third random boxes -- more detections than ground truths, so several
    detections land on one ground truth and tp < tpp."""
    c = MATCH_BY_NAME[name]
    rng = np.random.default_rng(9000 + c.seed)
    gt, det = _boxes(rng, c.ngt), _boxes(rng, c.ndet)
    gt[:, 4] = gt[:, 6] = 1.0
    if c.flavour == "disjoint":
        gt[:, 0] = 0.05 + 0.06 * np.arange(c.ngt)            # ground truths left of x = 0.5, detections right of it
        gt[:, 2] = 0.04
        gt[:, 5] = np.arange(c.ngt) % 2                      # classes 0 and 1 only
        det[:, 0] = rng.random(c.ndet) * 0.3 + 0.65
        det[:, 2] = 0.08
    elif c.ngt and c.ndet:
        if c.flavour in ("empty-class", "duplicates"):
            gt[:, 5] = np.arange(c.ngt) % 2
        src = rng.integers(0, c.ngt, c.ndet)
        copy = rng.random(c.ndet) < 2 / 3
        noisy = gt[src].copy()
        noisy[:, :2] += rng.normal(0, 0.03, (c.ndet, 2))
        noisy[:, 2:4] *= 1 + rng.normal(0, 0.15, (c.ndet, 2))
        det[copy, :4] = noisy[copy, :4]
        same = copy & (rng.random(c.ndet) < 0.8)
        det[same, 5] = gt[src[same], 5]
        if c.flavour in ("duplicates", "everything"):
            dup = (1, 4) if c.flavour == "duplicates" else (10, 200)
            gt[dup[1]] = gt[dup[0]]                          # a later copy of an earlier row: the first must win
            near = np.flatnonzero(copy)[:40]
            det[near, :4] = gt[dup[0], :4] * (1 + rng.normal(0, 0.05, (len(near), 4)))
            det[near, 5] = gt[dup[0], 5]
        if c.flavour == "everything":
            gt[240:246, 5] = -1
            gt[250:256, 5] = MATCH_CLASSES
            out = rng.choice(c.ndet, 40, replace=False)
            det[out[:20], 5] = -1
            det[out[20:], 5] = MATCH_CLASSES
            det[out[:10], :4] = gt[240 + np.arange(10) % 6, :4] * (1 + rng.normal(0, 0.03, (10, 4)))   # matched among themselves
    gt.setflags(write=False)
    det.setflags(write=False)
    return gt, det


@functools.lru_cache(maxsize=None)
def match_reference(name):
    c = MATCH_BY_NAME[name]
    return ref_match(*match_case(name), MATCH_CLASSES, c.thr)


# ---- ops.pr_curve ---------------------------------------------------------------------------------------------------
PR_NS = [1, 1023, 1024, 1025, 2500, 3100]
PR_NUM_GTS = [1, 300, 5000]
PR_KINDS = ["mixed", "none", "all", "ties", "nan"]


@functools.lru_cache(maxsize=None)
def pr_case(n, num_gts, kind):
    """(joint float64 [n], gid int32 [n], matched uint8 [n]), read-only. mixed: continuous scores, about half of the rows
    matched, ids uniform over the ground truths (several matched rows per id wherever n / 2 > num_gts); none / all: no
    row / every row matched; ties: scores from five values, so rows that differ in `matched` tie; nan: a seventh of the
    scores NaN and a few +inf."""
    rng = np.random.default_rng(100000 * PR_KINDS.index(kind) + 10 * n + PR_NUM_GTS.index(num_gts))
    joint = rng.random(n)
    gid = rng.integers(0, num_gts, n).astype(np.int32)
    matched = (rng.random(n) < 0.5).astype(np.uint8)
    if kind == "none":
        matched[:] = 0
    elif kind == "all":
        matched[:] = 1
    elif kind == "ties":
        joint = rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 0.9]), size=n)
    elif kind == "nan":
        joint[rng.choice(n, max(1, n // 7), replace=False)] = np.nan
        if n > 8:
            joint[rng.choice(n, 3, replace=False)] = np.inf
    for a in (joint, gid, matched):
        a.setflags(write=False)
    return joint, gid, matched


@functools.lru_cache(maxsize=None)
def pr_reference(n, num_gts, kind, mode):
    return ref_pr_curve(*pr_case(n, num_gts, kind), num_gts, mode)


# ---- the drop-in functions at real sizes ----------------------------------------------------------------------------
MANY_CLASSES, DENSE_CLASSES = 2, 3
DENSE_KW = dict(conf_threshold=0.5, nms_mode=0, max_per_img=100)
DENSE_THRESHOLDS = (0.1, 0.5)
TIES_KW = dict(max_per_img=5)


@functools.lru_cache(maxsize=None)
def many_inputs():
    """260 images, 2 classes: about 3000 detections and 700 ground truths per class (PRfunc defaults)"""
    return gen_inputs.measurement_inputs(seed=33, n_img=260, C=MANY_CLASSES)


@functools.lru_cache(maxsize=None)
def tied_inputs():
    """many_inputs() with every confidence -- the box confidence and the class probabilities, the two factors of the
    joint confidence -- rounded to one decimal: a few dozen distinct joint confidences for thousands of detections"""
    y_true, lv0, lv1 = many_inputs()
    out = []
    for lv in (lv0, lv1):
        v = lv.copy().reshape(*lv.shape[:3], -1, 5 + MANY_CLASSES)
        v[..., 4:] = np.round(v[..., 4:], 1)
        out.append(v.reshape(lv.shape))
    return y_true, out[0], out[1]


@functools.lru_cache(maxsize=None)
def dense_inputs(seed=44, n_img=2, g=20, A=3):
    """two images on a g x g grid with EVERY cell labelled (g * g ground truths per image) and uniform-noise predictions
    on two levels (g and g / 2): about 0.153 = (1 - ln 2) / 2 of the A * C * (g^2 + g^2 / 4) joint confidences pass 0.5"""
    C = DENSE_CLASSES
    rng = np.random.default_rng(seed)
    y_true = np.zeros((n_img, g, g, 5 + C))
    y_true[..., :2] = rng.random((n_img, g, g, 2))
    y_true[..., 2:4] = rng.random((n_img, g, g, 2)) * 0.3 + 0.08
    y_true[..., 4] = 1
    cls = rng.integers(0, C, (n_img, g, g))
    for c in range(C):
        y_true[..., 5 + c] = cls == c
    lv0 = rng.random((n_img, g, g, A * (5 + C)), dtype=np.float32)
    lv1 = rng.random((n_img, g // 2, g // 2, A * (5 + C)), dtype=np.float32)
    return y_true, lv0, lv1


def image_rows(y_true, preds, class_num, conf_threshold=0.05, nms_mode=1, nms_threshold=0.5, nms_sigma=0.5, version=3, **_):
    """the oracle's (ground-truth rows, detection rows) of every image"""
    return [OM._rows(y_true[i], [p[i] for p in preds], class_num, conf_threshold, nms_mode, nms_threshold, nms_sigma, version)
            for i in range(len(y_true))]


def size_stats(rows, class_num):
    """(most detections of an image, most ground truths of an image, detections per class over all images)"""
    per_class = np.zeros(class_num, dtype=np.int64)
    for _, det in rows:
        per_class += np.bincount(det[:, 5].astype("int"), minlength=class_num)[:class_num]
    return max(len(d) for _, d in rows), max(len(g) for g, _ in rows), per_class
