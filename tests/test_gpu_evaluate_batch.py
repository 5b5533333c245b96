"""Data-set evaluation on the device: the kernels of tf2_yolo_amd/csrc/measure.hip through ops (match_batch,
rank_desc_images, pr_curves) against the NumPy references of tests/measure_cases.py and against the per-image / per-class
front ends of the same kernels; measurement.Evaluator against the oracle and the reference's own outputs (golden), fed in chunks of 1,
7 and all images; Model.evaluate_detections against PRfunc / create_score_mat on predict's arrays. Every comparison is exact
(NaNs positionally), except best_iou against NumPy, where the existing kernel test allows the compiler's fused multiply-adds.

Shapes: image boundaries at rows 255 / 256 / 257 (a 256-thread workgroup straddles images), more than 256 ground truths and
more than 256 rows of one class in one image (a second tile), more than 2 x 1024 detections of one class (the scan carries)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_inputs                                    # noqa: E402
from make_measurement_golden import CLASS_NAMES, PR_CASES, SCORE_CASES   # noqa: E402

import measure_cases as MC                           # noqa: E402
import test_gpu_measurement as TM                    # noqa: E402  (its cached oracle runs and checks are shared, not redone)
from oracle import measurement as OM                  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = TM.GOLD
_eq = TM._eq


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the cases are read-only)


def _offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


# ---- ops.match_batch --------------------------------------------------------------------------------------------------
_NONE = np.zeros((0, 7))
MATCH_LAYOUTS = {
    # detections 255 | 1 | 1 | 0 | 700: image boundaries at rows 255, 256, 257; image 1 has no ground truth; image 3 is empty
    # between two populated ones (B = 5 with an image without detections); image 4 has 300 ground truths and the class ids
    # -1 and class_num on both sides
    "boundaries": lambda: [MC.match_case("gt7-det255"), (_NONE, MC.match_case("gt1-det1")[1]), MC.match_case("gt1-det1"),
                           (_NONE, _NONE), MC.match_case("gt300-det700")],
    # ground truths only | detections only | both, with duplicated ground-truth rows (exact IoU ties: the first wins)
    "one-sided": lambda: [MC.match_case("gt300-det0"), MC.match_case("gt0-det300"), MC.match_case("gt7-det256")],
}
GTS_SEEN = np.array([5, 0, 11], dtype=np.int64)


def _match_reference(images, C, thr, seen):
    """ref_match image by image; gid by the running-offset rule: best_gt + the class's ground truths in earlier images + seen,
    0 where the image has no ground truth of the class, best_gt alone for a class id outside [0, C)"""
    run, counts, cols = seen.copy(), np.zeros((C, 4), dtype=np.int64), []
    for gt, det in images:
        best_gt, matched, best_iou, cnt = MC.ref_match(gt, det, C, thr)
        gcls, dcls = gt[:, 5].astype("int"), det[:, 5].astype("int")
        here = np.bincount(gcls[(gcls >= 0) & (gcls < C)], minlength=C)
        gid = best_gt.copy()
        inside = (dcls >= 0) & (dcls < C)
        c = dcls[inside]
        gid[inside] = np.where(here[c] > 0, best_gt[inside] + run[c], 0)
        cols.append((best_gt, matched, best_iou, gid))
        run += here
        counts += cnt
    return [np.concatenate(col) for col in zip(*cols)], counts, run


@pytest.mark.parametrize("layout", list(MATCH_LAYOUTS))
def test_match_batch(layout):
    from tf2_yolo_amd import ops
    C, thr = MC.MATCH_CLASSES, 0.5
    images = MATCH_LAYOUTS[layout]()
    gt_sizes, det_sizes = [len(g) for g, _ in images], [len(d) for _, d in images]
    if layout == "boundaries":
        assert list(np.cumsum(det_sizes)[:3]) == [255, 256, 257] and max(gt_sizes) > 256 and len(images) == 5
        ids = np.concatenate([d[:, 5] for _, d in images])
        assert (ids == -1).any() and (ids == C).any()
    gt = _dev(np.concatenate([g for g, _ in images]))
    det = _dev(np.concatenate([d for _, d in images]))
    gt_off, det_off = _dev(_offsets(gt_sizes)), _dev(_offsets(det_sizes))
    (best_gt, matched, best_iou, gid), counts, seen_after = _match_reference(images, C, thr, GTS_SEEN)
    seen, acc = _dev(GTS_SEEN), torch.zeros((C, 4), device="cuda", dtype=torch.int64)
    g_best, g_matched, g_iou, g_gid = ops.match_batch(gt, gt_off, det, det_off, C, thr, seen, acc)
    assert (g_best.dtype, g_matched.dtype, g_iou.dtype, g_gid.dtype) == (torch.int32, torch.uint8, torch.float64, torch.int32)
    assert np.array_equal(g_best.cpu().numpy(), best_gt)
    assert np.array_equal(g_matched.cpu().numpy(), matched)
    assert np.array_equal(g_gid.cpu().numpy(), gid)
    assert np.array_equal(acc.cpu().numpy(), counts)
    assert np.array_equal(seen.cpu().numpy(), seen_after) and (seen_after > GTS_SEEN).all()
    err = np.abs(g_iou.cpu().numpy() - best_iou)
    assert (err <= 1e-12 * np.abs(best_iou)).all(), float(err.max())
    # and exactly what the per-image kernels give, image by image
    single = torch.zeros((C, 4), device="cuda", dtype=torch.int64)
    d0 = 0
    for g, d in images:
        s_best, s_matched, s_iou = ops.match_detections(_dev(g), _dev(d), C, thr, single)
        sl = slice(d0, d0 + len(d))
        assert torch.equal(s_best, g_best[sl]) and torch.equal(s_matched, g_matched[sl]) and torch.equal(s_iou, g_iou[sl])
        d0 += len(d)
    assert torch.equal(single, acc)
    # a second call accumulates: the counts double, the ids move on by the first call's ground truths
    again = ops.match_batch(gt, gt_off, det, det_off, C, thr, seen, acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * counts)
    assert np.array_equal(seen.cpu().numpy(), 2 * seen_after - GTS_SEEN)
    _, _, want_gid = _match_reference(images, C, thr, seen_after)[0][1:]
    assert np.array_equal(again[3].cpu().numpy(), want_gid) and torch.equal(again[0], g_best)


def test_match_batch_of_no_rows():
    from tf2_yolo_amd import ops
    none = torch.empty((0, 7), device="cuda", dtype=torch.float64)
    off = torch.zeros(4, device="cuda", dtype=torch.int32)
    seen, acc = _dev(GTS_SEEN), torch.zeros((3, 4), device="cuda", dtype=torch.int64)
    out = ops.match_batch(none, off, none, off, 3, 0.5, seen, acc)
    assert all(o.shape == (0,) for o in out) and not acc.any() and np.array_equal(seen.cpu().numpy(), GTS_SEEN)


# ---- ops.rank_desc_images ---------------------------------------------------------------------------------------------
RANK_LAYOUTS = {"second-tile": [300, 0, 257, 5], "boundaries": [255, 1, 1, 0, 300]}
RANK_CLASSES = 3


def _rank_case(sizes):
    """keys with long tie runs, -0.0 / 0.0, NaN and +inf; the first image has more than 256 rows of class 0"""
    rng = np.random.default_rng(sum(sizes))
    n = sum(sizes)
    key = rng.choice(np.array([0.125, 0.3, 0.5, 0.7, 0.9]), size=n)
    sel = rng.random(n) < 0.5
    key[sel] = rng.random(int(sel.sum()))
    sel = rng.random(n) < 0.2
    key[sel] = rng.choice(np.array([-0.0, 0.0, np.inf, -np.inf, np.nan]), size=int(sel.sum()))
    cls = rng.integers(0, RANK_CLASSES, n).astype(np.int32)
    if sizes[0] > 256:
        cls[:270] = 0
    img = np.repeat(np.arange(len(sizes)), sizes)
    return key, cls, img


@pytest.mark.parametrize("layout", list(RANK_LAYOUTS))
def test_rank_desc_images(layout):
    from tf2_yolo_amd import ops
    sizes = RANK_LAYOUTS[layout]
    key, cls, img = _rank_case(sizes)
    assert np.isnan(key).any() and np.isinf(key).any() and (np.signbit(key) & (key == 0)).any() and 0 in sizes
    off = _dev(_offsets(sizes))
    got = ops.rank_desc_images(_dev(key), _dev(cls), off).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, MC.ref_rank_desc(key, img * RANK_CLASSES + cls))
    if layout == "second-tile":
        assert np.bincount(img * RANK_CLASSES + cls).max() > 256 and got.max() > 256
    # one class per image, and the same ranks from the single-call kernel with the segment spelled out
    got = ops.rank_desc_images(_dev(key), None, off)
    assert np.array_equal(got.cpu().numpy(), MC.ref_rank_desc(key, img))
    assert torch.equal(got, ops.rank_desc(_dev(key), _dev(img.astype(np.int32))))


def test_rank_desc_images_of_nothing():
    from tf2_yolo_amd import ops
    off = torch.zeros(3, device="cuda", dtype=torch.int32)
    assert ops.rank_desc_images(torch.empty(0, dtype=torch.float64, device="cuda"), None, off).shape == (0,)


# ---- ops.pr_curves ----------------------------------------------------------------------------------------------------
PRC_ROWS = [300, 0, 2500, 200]          # class 1 has no detection and sits between populated classes; class 2: the scan carries
PRC_GTS = np.array([150, 40, 300, 0], dtype=np.int64)      # class 3 has detections and no ground truth


def _prc_case(kind):
    rng = np.random.default_rng(77 + (kind == "ties"))
    cls = np.repeat(np.arange(4), PRC_ROWS)
    cls = np.concatenate((cls, np.full(30, -1), np.full(30, 4)))          # rows the call passes over
    cls = rng.permutation(cls).astype(np.int32)
    n = len(cls)
    joint = rng.random(n)
    if kind == "ties":
        joint = rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 0.9]), size=n)
    gid = (rng.random(n) * np.maximum(PRC_GTS, 1)[cls.clip(0, 3)]).astype(np.int32)
    matched = (rng.random(n) < 0.5).astype(np.uint8)
    return joint, gid, matched, cls


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["mixed", "ties"])
def test_pr_curves(kind, mode):
    from tf2_yolo_amd import ops
    joint, gid, matched, cls = _prc_case(kind)
    assert PRC_ROWS[2] > 2 * MC.SCAN_CHUNK
    d_joint, d_gid, d_matched, d_cls = _dev(joint), _dev(gid), _dev(matched), _dev(cls)
    n = len(cls)
    for gts_total in (None, int(PRC_GTS.sum()) + 500):        # read from the device / a looser bound known on the host
        cls_off, prec, rec = ops.pr_curves(d_joint, d_gid, d_matched, d_cls, _dev(PRC_GTS), mode, gts_total=gts_total)
        assert prec.shape == rec.shape == (n + 4,) and cls_off.dtype == torch.int32
        off = cls_off.cpu().numpy()
        assert np.array_equal(off, _offsets(PRC_ROWS))
        prec, rec = prec.cpu().numpy(), rec.cpu().numpy()
        for c in (0, 2):
            rows = torch.from_numpy(np.flatnonzero(cls == c)).cuda()
            p, r = ops.pr_curve(d_joint[rows], d_gid[rows], d_matched[rows], int(PRC_GTS[c]), mode)
            first, m = off[c] + c, PRC_ROWS[c] + 1
            assert np.array_equal(prec[first:first + m], p.cpu().numpy()), c
            assert np.array_equal(rec[first:first + m], r.cpu().numpy()), c
            sel = cls == c
            want_p, want_r = MC.ref_pr_curve(joint[sel], gid[sel], matched[sel], int(PRC_GTS[c]), mode)
            assert np.array_equal(prec[first:first + m], want_p) and np.array_equal(rec[first:first + m], want_r), c


def test_pr_curves_of_nothing_and_rejections():
    from tf2_yolo_amd import ops
    from tf2_yolo_amd._lib import YoloHipError
    e = lambda dt: torch.empty(0, device="cuda", dtype=dt)
    cls_off, prec, rec = ops.pr_curves(e(torch.float64), e(torch.int32), e(torch.uint8), e(torch.int32), _dev(PRC_GTS), 2)
    assert not cls_off.any() and cls_off.shape == (5,) and prec.shape == (4,)
    joint, gid, matched, cls = (_dev(a) for a in _prc_case("mixed"))
    with pytest.raises(YoloHipError):
        ops.pr_curves(joint, gid, matched, cls, _dev(PRC_GTS), 3)
    with pytest.raises(YoloHipError):
        ops.pr_curves(joint, gid, matched, cls[:-1], _dev(PRC_GTS), 2)


# ---- measurement.Evaluator --------------------------------------------------------------------------------------------
def _feed(ev, arrays, chunk):
    n = len(arrays[0])
    chunk = n if chunk is None else chunk
    for i in range(0, n, chunk):
        ev.update(*[a[i:i + chunk] for a in arrays])
    assert ev.images == n
    return ev


def _check_evaluator(ev, recs, gts, counts, order=None):
    """curves and mAPs (all four modes) in the three precision modes from ONE evaluator, and its score tables"""
    for pm in (0, 1, 2):
        ev.precision_mode = pm
        TM._check_prfunc(ev.prfunc(), *TM._oracle_curves(recs, gts, pm, order))
        TM._check_score_mat(ev.score_mat(pm), counts, pm)
    ev.precision_mode = 1
    TM._check_score_mat(ev.score_mat(), counts, 1)          # None: the evaluator's own


CHUNKS = [1, 7, None]


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk-{c or 'all'}")
def test_evaluator_many_images(chunk):
    """260 images, about 3000 detections per class (the scan of pr_curves carries), PRfunc's defaults"""
    from utils.measurement import Evaluator
    ev = _feed(Evaluator(["a", "b"], version=3), MC.many_inputs(), chunk)
    recs, gts = TM._oracle_records("many_inputs")
    assert all(len(rec) > 2 * MC.SCAN_CHUNK for rec in recs)
    _check_evaluator(ev, recs, gts, TM._oracle_counts("many_inputs", conf_threshold=0.05, nms_mode=1))


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk-{c or 'all'}")
@pytest.mark.parametrize("iou_threshold", MC.DENSE_THRESHOLDS)
def test_evaluator_dense_images(iou_threshold, chunk):
    """400 ground truths and about 700 detections per image; the cap of 100 per image and class really cuts"""
    from utils.measurement import Evaluator
    ev = _feed(Evaluator(["a", "b", "c"], version=3, iou_threshold=iou_threshold, **MC.DENSE_KW), MC.dense_inputs(), chunk)
    recs, gts = TM._oracle_records("dense_inputs", iou_threshold=iou_threshold, **MC.DENSE_KW)
    assert [len(rec) for rec in recs] == [2 * MC.DENSE_KW["max_per_img"]] * 3
    counts = TM._oracle_counts("dense_inputs", conf_threshold=MC.DENSE_KW["conf_threshold"], nms_mode=0, iou_threshold=iou_threshold)
    assert (counts[:, 0] > 2 * MC.DENSE_KW["max_per_img"]).all()
    _check_evaluator(ev, recs, gts, counts)


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk-{c or 'all'}")
def test_evaluator_tied_confidences(chunk):
    """a few dozen distinct joint confidences; a cap of 5 per image and class cuts inside tie runs: the later detection first,
    in the cut and on the curve, whatever the chunking"""
    from utils.measurement import Evaluator
    ev = _feed(Evaluator(["a", "b"], version=3, **MC.TIES_KW), MC.tied_inputs(), chunk)
    recs, gts = TM._oracle_records("tied_inputs", order=MC.ref_order, **MC.TIES_KW)
    _check_evaluator(ev, recs, gts, TM._oracle_counts("tied_inputs", conf_threshold=0.05, nms_mode=1), MC.ref_order)


@pytest.mark.parametrize("chunk", [3, None], ids=["chunk-3", "chunk-all"])
@pytest.mark.parametrize("key,kw", PR_CASES)
def test_evaluator_curves_match_reference(key, kw, chunk):
    """the reference's own curves, mAPs and calls (golden); CUDA tensors in place of NumPy arrays"""
    from utils.measurement import Evaluator
    arrays = gen_inputs.measurement_inputs()
    if chunk is None:
        arrays = [torch.from_numpy(a).cuda() for a in arrays]
    f = _feed(Evaluator(CLASS_NAMES, version=3, **kw), arrays, chunk).prfunc()
    for c in range(3):
        assert _eq(f.precisions[c], GOLD[f"{key}_prec{c}"]) and _eq(f.recalls[c], GOLD[f"{key}_rec{c}"]), (key, c)
    for mode in TM.MAP_MODES:
        m = f.get_map(mode)
        assert list(m.index) == CLASS_NAMES + ["mAP"] and list(m.columns) == ["ap"]
        assert _eq(m["ap"].to_numpy(), GOLD[f"{key}_map_{mode}"]), (key, mode)
    assert _eq([[f(r, c) for r in (0.0, 0.3, 0.55, 0.9)] for c in range(3)], GOLD[f"{key}_call"])
    with pytest.raises(IndexError):
        f(0.5, 3)


@pytest.mark.parametrize("chunk", [3, None], ids=["chunk-3", "chunk-all"])
@pytest.mark.parametrize("key,kw", SCORE_CASES)
def test_evaluator_score_table_matches_reference(key, kw, chunk):
    from utils.measurement import Evaluator
    t = _feed(Evaluator(CLASS_NAMES, version=3, max_per_img=None, **kw), gen_inputs.measurement_inputs(), chunk).score_mat()
    assert list(t.columns) == ["precision", "recall", "F1-score", "gts", "dets"] and list(t.index) == CLASS_NAMES
    for col in ("precision", "recall", "F1-score", "gts", "dets"):
        assert _eq(t[col].to_numpy(), GOLD[f"{key}_{col}"]), (key, col)


@pytest.mark.parametrize("version,levels", [(2, 1), (4, 2)])
def test_evaluator_other_versions(version, levels):
    from utils.measurement import Evaluator
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    preds = (lv0, lv1)[:levels]
    kw = dict(SCORE_CASES[1][1])
    pm = kw.pop("precision_mode")
    ev = _feed(Evaluator(CLASS_NAMES, version=version, precision_mode=pm, **kw), (y_true,) + preds, 3)
    TM._check_score_mat(ev.score_mat(), OM.score_counts(y_true, preds, 3, version=version, **kw), pm)
    for _, kw in PR_CASES:
        ev = _feed(Evaluator(CLASS_NAMES, version=version, **kw), (y_true,) + preds, 3)
        TM._check_prfunc(ev.prfunc(), *OM.pr_curves(y_true, preds, 3, version=version, **kw))


def test_evaluator_without_classes_or_detections():
    from utils.measurement import Evaluator
    y_true, lv0, lv1 = gen_inputs.measurement_inputs(seed=3, n_img=2, C=3)
    none = _feed(Evaluator([], version=3), (y_true, lv0, lv1), None)
    assert none.score_mat().shape == (0, 5) and none.prfunc().precisions == []
    ev = _feed(Evaluator(["a", "b", "c"], version=3), (y_true, lv0 * 0, lv1 * 0), 1)
    t, f = ev.score_mat(), ev.prfunc()
    assert (t["dets"].to_numpy() == 0).all() and (t["gts"].to_numpy() > 0).any() and np.isnan(t["precision"].to_numpy()).all()
    assert all(len(p) == 1 and p[0] == 0 for p in f.precisions) and f.get_map("voc2007")["ap"].to_numpy()[-1] == 0


# ---- Model.evaluate_detections ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tiny-v3-64", "v2-64"])
def net_case(request):
    import gc
    from test_gpu_predict_fp16 import _setup
    kw = dict(version=3, hw=64, N=5, tiny=True) if request.param == "tiny-v3-64" else dict(version=2, hw=64, N=5)
    y, model, fwd, x = _setup(**kw)
    assert len(x) == 5
    yield model, x
    del y, model
    gc.collect()
    torch.cuda.empty_cache()


def _listed(p):
    return p if isinstance(p, list) else [p]


def _labels_from(pred, C):
    """(a label tensor, a confidence threshold) made from predict's arrays so that the evaluation has something to count:
    the threshold is the 300th largest conf * prob product of the batch; a cell of the last level whose first anchor passes
    it becomes a ground truth with that box and its best class"""
    prods = []
    for lv in pred:
        t = lv.reshape(*lv.shape[:3], lv.shape[-1] // (5 + C), 5 + C)
        prods.append((t[..., 4:5] * t[..., 5:]).ravel())
    thr = float(np.sort(np.concatenate(prods))[-300])
    lv = pred[-1]
    t = lv.reshape(*lv.shape[:3], lv.shape[-1] // (5 + C), 5 + C)[..., 0, :].astype(np.float64)
    hit = (t[..., 4:5] * t[..., 5:]).max(axis=-1) >= thr
    y = t.copy()
    y[..., 4] = hit
    y[..., 5:] = np.eye(C)[t[..., 5:].argmax(axis=-1)] * hit[..., None]
    return y, thr


def _check_model(model, x, precision, rescale=None):
    from utils.measurement import PRfunc, create_score_mat
    C = next(u.C for u in model.net.units if u.kind == "head")
    names = [f"k{i}" for i in range(C)]
    pkw = dict(batch_size=2, precision=precision, **({} if rescale is None else dict(rescale=rescale)))
    pred = _listed(model.predict(x, **pkw))
    y, thr = _labels_from(pred, C)
    kw = dict(conf_threshold=thr, nms_mode=1, nms_threshold=0.45, iou_threshold=0.5)
    for max_per_img in (100, 3):
        ev = model.evaluate_detections(x, y, names, max_per_img=max_per_img, precision_mode=1, **pkw, **kw)
        assert ev.images == 5
        t, want_t = ev.score_mat(), create_score_mat(y, *pred, class_names=names, precision_mode=1, version=model.version, **kw)
        assert t["gts"].sum() > 0 and t["dets"].sum() >= t["gts"].sum() and (t["recall"].to_numpy() > 0).any()
        assert list(t.index) == names and all(_eq(t[col].to_numpy(), want_t[col].to_numpy()) for col in want_t.columns)
        f = ev.prfunc()
        want = PRfunc(y, *pred, class_names=names, precision_mode=1, max_per_img=max_per_img, version=model.version, **kw)
        assert len(f.precisions) == C and sum(len(p) for p in f.precisions) > C
        assert all(_eq(a, b) for a, b in zip(f.precisions, want.precisions)) and all(_eq(a, b) for a, b in zip(f.recalls, want.recalls))
        assert _eq(f.get_map("area")["ap"].to_numpy(), want.get_map("area")["ap"].to_numpy())
    return y, pred, kw, names


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_evaluate_detections(net_case, precision):
    """len(x) = 5 with batch_size = 2: three chunks, the last one short; the head buffers go to the evaluator in place"""
    model, x = net_case
    y, pred, kw, names = _check_model(model, x, precision)
    # a list of label levels stands for its last one; a Sequence of (img, label) batches brings its own labels
    want = model.evaluate_detections(x, y, names, batch_size=2, precision=precision, **kw).score_mat()
    junk = np.zeros((5, 1, 1, y.shape[-1]))
    seq = [(x[i:i + 2], [junk[i:i + 2], y[i:i + 2]]) for i in range(0, 5, 2)]
    for got in (model.evaluate_detections(x, [junk, y], names, batch_size=2, precision=precision, **kw),
                model.evaluate_detections(seq, None, names, precision=precision, **kw)):
        assert got.score_mat().equals(want)
    again = _listed(model.predict(x, batch_size=2, precision=precision))
    assert all(np.array_equal(a, b) for a, b in zip(pred, again))


def test_model_evaluate_detections_of_raw_pixels(net_case):
    model, _ = net_case
    x8 = np.random.default_rng(5).integers(0, 256, (5, 64, 64, 3), dtype=np.uint8)
    _check_model(model, x8, "fp32", rescale=1 / 255)


def test_model_evaluate_detections_refusals(net_case):
    model, x = net_case
    C = next(u.C for u in model.net.units if u.kind == "head")
    names = [f"k{i}" for i in range(C)]
    y = np.zeros((5, 2, 2, 5 + C))
    with pytest.raises(ValueError, match="class_names"):
        model.evaluate_detections(x, y, names + ["one more"])
    with pytest.raises(ValueError, match="nms_mode"):
        model.evaluate_detections(x, y, names, nms_mode=4)
    with pytest.raises(ValueError, match="precision"):
        model.evaluate_detections(x, y, names, precision="int8")
    with pytest.raises(ValueError, match="different numbers"):
        model.evaluate_detections(x, y[:4], names)
    with pytest.raises(ValueError, match="Sequence"):
        model.evaluate_detections(x, None, names)
    version, model.version = model.version, 0
    try:
        with pytest.raises(ValueError, match="classifier"):
            model.evaluate_detections(x, y, names)
    finally:
        model.version = version
