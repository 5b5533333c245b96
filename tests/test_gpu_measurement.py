"""GPU evaluation path (utils.measurement drop-in: create_score_mat, PRfunc) against the outputs of the
reference's own utils/measurement.py (golden) and against the NumPy oracle on further inputs. Bit-exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_inputs                                    # noqa: E402
from make_measurement_golden import CLASS_NAMES, PR_CASES, SCORE_CASES   # noqa: E402

from oracle import measurement as OM                  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "measurement_golden.npz"))


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("key,kw", SCORE_CASES)
def test_create_score_mat_matches_reference(key, kw):
    from utils.measurement import create_score_mat
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    t = create_score_mat(y_true, lv0, lv1, class_names=CLASS_NAMES, version=3, **kw)
    assert list(t.columns) == ["precision", "recall", "F1-score", "gts", "dets"] and list(t.index) == CLASS_NAMES
    for col in ("precision", "recall", "F1-score", "gts", "dets"):
        assert _eq(t[col].to_numpy(), GOLD[f"{key}_{col}"]), (key, col)


@pytest.mark.parametrize("key,kw", PR_CASES)
def test_prfunc_matches_reference(key, kw):
    from utils.measurement import PRfunc
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    f = PRfunc(y_true, lv0, lv1, class_names=CLASS_NAMES, version=3, **kw)
    for c in range(3):
        assert _eq(f.precisions[c], GOLD[f"{key}_prec{c}"]), (key, c)
        assert _eq(f.recalls[c], GOLD[f"{key}_rec{c}"]), (key, c)
    for mode in ("voc2007", "voc2012", "area", "smootharea"):
        m = f.get_map(mode)
        assert list(m.index) == CLASS_NAMES + ["mAP"] and list(m.columns) == ["ap"]
        assert _eq(m["ap"].to_numpy(), GOLD[f"{key}_map_{mode}"]), (key, mode)
    calls = [[f(r, c) for r in (0.0, 0.3, 0.55, 0.9)] for c in range(3)]
    assert _eq(calls, GOLD[f"{key}_call"])
    with pytest.raises(IndexError):
        f(0.5, 3)


def test_larger_set_against_oracle():
    """more images / classes than the golden fixture, soft-NMS, a tight per-image cap"""
    from utils.measurement import PRfunc, create_score_mat
    y_true, lv0, lv1 = gen_inputs.measurement_inputs(seed=21, n_img=40, C=5, A=3, g=8)
    names = [f"k{i}" for i in range(5)]
    kw = dict(conf_threshold=0.2, nms_mode=2, nms_threshold=0.5, nms_sigma=0.4, iou_threshold=0.5)
    t = create_score_mat(y_true, lv0, lv1, class_names=names, precision_mode=1, version=3, **kw)
    counts = OM.score_counts(y_true, (lv0, lv1), 5, version=3, **kw)
    p, r, f1 = OM.score_table(counts, 1)
    assert _eq(t["precision"].to_numpy(), p) and _eq(t["recall"].to_numpy(), r) and _eq(t["F1-score"].to_numpy(), f1)
    f = PRfunc(y_true, lv0, lv1, class_names=names, precision_mode=2, max_per_img=3, version=3, **kw)
    ps, rs = OM.pr_curves(y_true, (lv0, lv1), 5, precision_mode=2, max_per_img=3, version=3, **kw)
    for c in range(5):
        assert _eq(f.precisions[c], ps[c]) and _eq(f.recalls[c], rs[c]), c
    assert _eq(f.get_map("area")["ap"].to_numpy(), OM.average_precisions(ps, rs, "area"))


def test_empty_corners():
    """no detections at all / a class nobody predicts: defined results instead of the reference's NameError"""
    from utils.measurement import PRfunc, create_score_mat
    y_true, lv0, lv1 = gen_inputs.measurement_inputs(seed=3, n_img=2, C=3)
    t = create_score_mat(y_true, lv0 * 0, lv1 * 0, class_names=["a", "b", "c"], version=3)
    assert (t["dets"].to_numpy() == 0).all() and np.isnan(t["precision"].to_numpy()).all()
    f = PRfunc(y_true, lv0 * 0, lv1 * 0, class_names=["a", "b", "c"], version=3)
    assert all(len(p) == 1 and p[0] == 0 for p in f.precisions)
    assert f.get_map("voc2007")["ap"].to_numpy()[-1] == 0


def test_detection_writers_match_reference_files(tmp_path):
    """array_to_json / array_to_xml: byte-identical files (the json after undoing the `np.float64(...)`
    wrappers that the reference's str(dict) leaks under NumPy 2 -- the numbers inside are identical)"""
    import json
    import re
    from make_writers_golden import CASES, IMG_SIZE, NAMES
    from utils.tools import array_to_json, array_to_xml
    gold = np.load(os.path.join(HERE, "golden", "writers_golden.npz"))
    _, lv0, lv1 = gen_inputs.measurement_inputs()
    for key, img, kw in CASES:
        pj, px = str(tmp_path / (key + ".json")), str(tmp_path / (key + ".xml"))
        array_to_json(pj, IMG_SIZE, lv0[img], lv1[img], class_names=NAMES, version=3, **kw)
        array_to_xml(px, IMG_SIZE, lv0[img], lv1[img], class_names=NAMES, version=3, **kw)
        want_json = re.sub(rb"np\.float64\(([^)]*)\)", rb"\1", gold[key + "_json"].tobytes())
        assert open(pj, "rb").read() == want_json, key
        assert open(px, "rb").read() == gold[key + "_xml"].tobytes(), key
        json.loads(open(pj, encoding="big5").read())   # and it is json


# ---- real sizes: past one tile of every kernel of measure.hip (tests/measure_cases.py; its GPU-free guards are in
# tests/test_measure_cases_cpu.py) ----
import functools                                     # noqa: E402

import measure_cases as MC                           # noqa: E402

MAP_MODES = ("voc2007", "voc2012", "area", "smootharea")


def _check_prfunc(f, ps, rs):
    assert len(f.precisions) == len(ps)
    for c in range(len(ps)):
        assert _eq(f.precisions[c], ps[c]) and _eq(f.recalls[c], rs[c]), c
    for mode in MAP_MODES:
        assert _eq(f.get_map(mode)["ap"].to_numpy(), OM.average_precisions(ps, rs, mode)), mode


def _check_score_mat(t, counts, precision_mode):
    p, r, f1 = OM.score_table(counts, precision_mode)
    assert _eq(t["precision"].to_numpy(), p) and _eq(t["recall"].to_numpy(), r) and _eq(t["F1-score"].to_numpy(), f1)
    assert np.array_equal(t["gts"].to_numpy(), counts[:, 1]) and np.array_equal(t["dets"].to_numpy(), counts[:, 0])


@functools.lru_cache(maxsize=None)
def _oracle_records(fixture, **kw):
    """the oracle's per-class records and ground-truth counts, once per fixture (the precision mode only enters the curve)"""
    y_true, lv0, lv1 = getattr(MC, fixture)()
    return OM.class_records(y_true, (lv0, lv1), y_true.shape[-1] - 5, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_counts(fixture, **kw):
    y_true, lv0, lv1 = getattr(MC, fixture)()
    return OM.score_counts(y_true, (lv0, lv1), y_true.shape[-1] - 5, **kw)


def _oracle_curves(recs, gts, precision_mode, order=None):
    curves = [OM.curve_from_records(rec, g, precision_mode, None if order is None else order(rec[:, 0]))
              for rec, g in zip(recs, gts)]
    return [p for p, _ in curves], [r for _, r in curves]


@pytest.mark.parametrize("precision_mode", [0, 1, 2])
def test_many_images_against_oracle(precision_mode):
    """260 images, about 3000 detections per class: four chunks of the PR scan with its (tpp, tp) carry, twelve tiles and
    workgroups of the rank kernel, PRfunc's defaults"""
    from utils.measurement import PRfunc, create_score_mat
    y_true, lv0, lv1 = MC.many_inputs()
    names = ["a", "b"]
    f = PRfunc(y_true, lv0, lv1, class_names=names, precision_mode=precision_mode, version=3)
    recs, gts = _oracle_records("many_inputs")
    assert all(len(rec) > 2 * MC.SCAN_CHUNK for rec in recs)
    _check_prfunc(f, *_oracle_curves(recs, gts, precision_mode))
    t = create_score_mat(y_true, lv0, lv1, class_names=names, precision_mode=precision_mode, version=3)
    _check_score_mat(t, _oracle_counts("many_inputs"), precision_mode)


@pytest.mark.parametrize("iou_threshold", MC.DENSE_THRESHOLDS)
def test_dense_images_against_oracle(iou_threshold):
    """two images with 400 ground truths and about 700 detections each: the second and third workgroup of mb_match_kernel,
    the second workgroup of mb_distinct_kernel, three rank tiles, and a per-image cap of 100 that really cuts (more than 200
    detections per class and image)"""
    from utils.measurement import PRfunc, create_score_mat
    y_true, lv0, lv1 = MC.dense_inputs()
    names = ["a", "b", "c"]
    recs, gts = _oracle_records("dense_inputs", iou_threshold=iou_threshold, **MC.DENSE_KW)
    assert [len(rec) for rec in recs] == [2 * MC.DENSE_KW["max_per_img"]] * 3
    for precision_mode in (0, 1, 2):
        f = PRfunc(y_true, lv0, lv1, class_names=names, iou_threshold=iou_threshold, precision_mode=precision_mode,
                   version=3, **MC.DENSE_KW)
        _check_prfunc(f, *_oracle_curves(recs, gts, precision_mode))
    kw = dict(conf_threshold=MC.DENSE_KW["conf_threshold"], nms_mode=0, iou_threshold=iou_threshold)
    counts = _oracle_counts("dense_inputs", **kw)
    assert (counts[:, 1] > 100).all() and (counts[:, 3] < counts[:, 2]).all() and (counts[:, 3] > 0).all()
    for precision_mode in (0, 1, 2):
        t = create_score_mat(y_true, lv0, lv1, class_names=names, precision_mode=precision_mode, version=3, **kw)
        _check_score_mat(t, counts, precision_mode)


@pytest.mark.parametrize("precision_mode", [0, 2])
def test_tied_confidences_end_to_end(precision_mode):
    """every confidence rounded to one decimal: thousands of detections share a few dozen joint confidences, and a cap of
    5 per image and class cuts inside tie runs. The rule -- the later detection first, in the cut and on the curve --
    against the oracle with ref_order in place of the reference's unstable np.argsort"""
    from utils.measurement import PRfunc
    y_true, lv0, lv1 = MC.tied_inputs()
    f = PRfunc(y_true, lv0, lv1, class_names=["a", "b"], precision_mode=precision_mode, version=3, **MC.TIES_KW)
    recs, gts = _oracle_records("tied_inputs", order=MC.ref_order, **MC.TIES_KW)
    _check_prfunc(f, *_oracle_curves(recs, gts, precision_mode, MC.ref_order))


@pytest.mark.parametrize("version,levels", [(2, 1), (4, 2)])
def test_other_versions_against_oracle(version, levels):
    """version 2 (one level) and version 4 with the golden fixture's sizes"""
    from utils.measurement import PRfunc, create_score_mat
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    preds = (lv0, lv1)[:levels]
    kw = dict(SCORE_CASES[1][1])
    pm = kw.pop("precision_mode")
    t = create_score_mat(y_true, *preds, class_names=CLASS_NAMES, precision_mode=pm, version=version, **kw)
    _check_score_mat(t, OM.score_counts(y_true, preds, 3, version=version, **kw), pm)
    for _, kw in PR_CASES:
        f = PRfunc(y_true, *preds, class_names=CLASS_NAMES, version=version, **kw)
        _check_prfunc(f, *OM.pr_curves(y_true, preds, 3, version=version, **kw))


def test_nan_confidence_does_not_pass_decode():
    """A NaN prediction confidence never reaches the evaluation kernels through the drop-in functions: decode keeps a
    candidate when `conf * prob >= threshold`, which is false for NaN -- on the device as in the reference's np.where. So
    the result equals the oracle's on the same input and equals the result with that confidence set to 0. NaN keys are
    therefore tested at the kernel level (tests/test_gpu_measure_kernels.py: yolo_rank_desc and yolo_pr_curve are a raw
    C-ABI and take any keys)."""
    from utils.measurement import PRfunc
    y_true, lv0, lv1 = gen_inputs.measurement_inputs()
    kw = dict(PR_CASES[0][1])
    v = lv0.copy().reshape(*lv0.shape[:3], 3, 8)
    b, y, x, a = (int(i[0]) for i in np.nonzero(v[..., 4] > 0.5))       # a box that is a detection in the fixture
    zero = v.copy()
    v[b, y, x, a, 4] = np.nan
    zero[b, y, x, a, 4] = 0.0
    f = PRfunc(y_true, v.reshape(lv0.shape), lv1, class_names=CLASS_NAMES, version=3, **kw)
    ps, rs = OM.pr_curves(y_true, (v.reshape(lv0.shape), lv1), 3, version=3, **kw)
    _check_prfunc(f, ps, rs)
    ps0, rs0 = OM.pr_curves(y_true, (zero.reshape(lv0.shape), lv1), 3, version=3, **kw)
    assert all(np.isfinite(p).all() for p in ps) and all(_eq(p, q) for p, q in zip(ps, ps0))
    assert any(not _eq(ps[c], GOLD[f"p0_prec{c}"]) for c in range(3))                   # and the row is gone
