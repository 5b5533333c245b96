"""Non-square grids without a GPU.

1. The inputs of the non-square loss / metrics / loss-side IoU tests (tests/nonsquare_cases.py) tell a height / width
   mix-up from the truth: on the float64 oracle, the same inputs evaluated with the two grid divisors swapped (tensor
   layout kept), and with the labels' cell axes transposed, give a loss value, a gradient and metrics that are at least
   100 x the GPU tests' tolerance (1e-4 of the tensor's scale, tests/test_gpu_loss.py:check) away from the right ones.
   A condition on the inputs, not a measurement: a kernel that mixed the two up could not pass the GPU test.
   obj_acc and class_acc never read the grid divisors (oracle/metrics.py), so for them only the transposed labels apply.
2. oracle/tools.py, oracle/measurement.py and tf2_yolo_amd/labels.py reproduce what the reference's own NumPy code gives
   on non-square grids (tests/golden/nonsquare_golden.npz, made by tests/golden/make_nonsquare_golden.py), bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_inputs  # noqa: E402
import nonsquare_cases as NS  # noqa: E402

from oracle import losses as OL  # noqa: E402
from oracle import measurement as OMS  # noqa: E402
from oracle import metrics as OM  # noqa: E402
from oracle import tools as T  # noqa: E402

TOL = 1e-4           # tests/test_gpu_loss.py
MARGIN = 100 * TOL


def _value_and_grad(fn, yt, yp):
    p = torch.tensor(yp, dtype=torch.float64, requires_grad=True)
    v = fn(torch.tensor(yt, dtype=torch.float64), p)
    v.backward()
    return v.item(), p.grad


def _swap_divisors(monkeypatch):
    """the oracle's IoU divides x by gh and y by gw; the tensors keep their layout"""
    real = OL.cal_iou
    swapped = lambda t, p, grid_shape, return_ciou=False: real(t, p, (grid_shape[1], grid_shape[0]), return_ciou)
    monkeypatch.setattr(OL, "cal_iou", swapped)
    monkeypatch.setattr(OM, "cal_iou", swapped)


@pytest.mark.parametrize("case", NS.LOSS_CASES, ids=[c["id"] for c in NS.LOSS_CASES])
def test_loss_inputs_tell_a_transpose_from_the_truth(case, monkeypatch):
    yt, yp = NS.build(case)
    fn = NS.oracle_loss(case)
    v, g = _value_and_grad(fn, yt, yp)
    vt, gt = _value_and_grad(fn, NS.transpose_truth(yt), yp)
    _swap_divisors(monkeypatch)
    vs, gs = _value_and_grad(NS.oracle_loss(case), yt, yp)
    gscale = g.abs().max().item()
    margins = {"value, divisors swapped": abs(vs - v) / max(abs(v), 1.0), "gradient, divisors swapped": (gs - g).abs().max().item() / gscale,
               "value, labels transposed": abs(vt - v) / max(abs(v), 1.0), "gradient, labels transposed": (gt - g).abs().max().item() / gscale}
    print("NONSQUARE_MARGIN", case["id"], {k: round(m / TOL, 1) for k, m in margins.items()}, "x TOL")
    for k, m in margins.items():
        assert m >= MARGIN, (case["id"], k, m)


@pytest.mark.parametrize("case", NS.METRIC_CASES, ids=[c["id"] for c in NS.METRIC_CASES])
def test_metric_inputs_tell_a_transpose_from_the_truth(case, monkeypatch):
    yt, yp = NS.build(case)
    ref = NS.oracle_metrics(case, yt, yp)
    tr = NS.oracle_metrics(case, NS.transpose_truth(yt), yp)
    _swap_divisors(monkeypatch)
    sw = NS.oracle_metrics(case, yt, yp)
    names = ["obj_acc", "mean_iou", "class_acc", "recall"]
    print("NONSQUARE_MARGIN metrics", case["id"], dict(zip(names, ref)), "swapped", dict(zip(names, sw)), "transposed", dict(zip(names, tr)))
    assert sw[0] == ref[0] and sw[2] == ref[2]          # (no divisor in them)
    for i in (1, 3):
        assert abs(sw[i] - ref[i]) >= MARGIN, (names[i], sw[i], ref[i])
    for i in range(4):
        assert abs(tr[i] - ref[i]) >= MARGIN, (names[i], tr[i], ref[i])


@pytest.mark.parametrize("grid,ciou", NS.IOU_CASES, ids=[f"{g[0]}x{g[1]}-{'ciou' if c else 'iou'}" for g, c in NS.IOU_CASES])
def test_iou_inputs_tell_swapped_divisors_from_the_truth(grid, ciou):
    t, p = NS.iou_operands(grid)
    t64, p64 = torch.tensor(t, dtype=torch.float64), torch.tensor(p, dtype=torch.float64)
    ref = OL.cal_iou(t64, p64, grid, return_ciou=ciou)
    sw = OL.cal_iou(t64, p64, grid[::-1], return_ciou=ciou)
    for a, b in zip(ref if ciou else [ref], sw if ciou else [sw]):
        d = (a - b).abs()
        print("NONSQUARE_MARGIN cal_iou", grid, ciou, round(d.max().item() / TOL, 1), "x TOL")
        assert d.max().item() >= MARGIN * a.abs().max().item()
        assert (d >= MARGIN).float().mean().item() > 0.1         # not one lucky element: a tenth of them


# ---- the NumPy oracle against the reference's own outputs on non-square grids ----
G = np.load(os.path.join(HERE, "golden", "nonsquare_golden.npz"))
CASES = list(gen_inputs.nonsquare_decode_cases())


@pytest.mark.parametrize("key,C,thr,lv", CASES, ids=[c[0] for c in CASES])
def test_decode_and_nms_match_reference(key, C, thr, lv):
    dec = T.decode(*lv, class_num=C, threshold=thr, version=3)
    ref = G[f"{key}_decode"]
    assert len(ref) > 20 and dec.shape == ref.shape and np.array_equal(dec, ref)
    assert np.array_equal(T.nms(dec, class_num=C, nms_threshold=0.5), G[f"{key}_nms"])
    assert np.array_equal(T.nms(dec, class_num=C, nms_threshold=0.5, iou_mode=2), G[f"{key}_diou"])
    assert np.array_equal(T.soft_nms(dec, class_num=C, nms_threshold=0.5, conf_threshold=thr, sigma=0.5), G[f"{key}_soft"])


def test_decode_v1_v2_labels_and_class_weights_match_reference():
    m = gen_inputs.nonsquare_misc_inputs()
    assert np.array_equal(T.decode(m["v1_lv"], class_num=4, threshold=0.4, version=1), G["v1_decode"]) and len(G["v1_decode"]) > 5
    assert np.array_equal(T.decode(m["v2_lv"], class_num=20, threshold=0.8, version=2), G["v2_decode"]) and len(G["v2_decode"]) > 5
    lab = m["label12x20"]
    assert np.array_equal(T.decode(lab[0], class_num=3, threshold=0.5, version=3), G["label12x20_decode"])
    l6 = T.down2xlabel(lab)
    l3 = T.down2xlabel(l6)
    assert l6.shape == (2, 6, 10, 8) and l3.shape == (2, 3, 5, 8)
    assert np.array_equal(l6, G["label6x10"]) and np.array_equal(l3, G["label3x5"])
    assert np.array_equal(T.get_class_weight(lab[..., 4:5], "binary"), G["binary_weight"])
    for meth in ("alpha", "log", "effective"):
        assert np.array_equal(T.get_class_weight(lab[..., 5:], meth), G[f"class_weight_{meth}"])
    # the product's host-side label code (tf2_yolo_amd/labels.py) gives the same tensors
    from tf2_yolo_amd import labels
    assert np.array_equal(labels.down2xlabel(lab), G["label6x10"])
    assert np.array_equal(labels.down2xlabel(labels.down2xlabel(lab)), G["label3x5"])
    for meth in ("alpha", "log", "effective"):
        assert np.array_equal(labels.get_class_weight(lab[..., 5:], meth), G[f"class_weight_{meth}"])


def test_encoder_oracle_and_host_code_agree_on_non_square_images():
    from tf2_yolo_amd import labels
    for hw, grid, boxes, classes in gen_inputs.nonsquare_encoder_cases():
        for b, c in zip(boxes, classes):
            ref = T.encode_boxes(b, c, hw, grid, 4)
            assert ref.shape == (*grid, 9) and np.array_equal(labels.encode_boxes(b, c, hw, grid, 4), ref)
    # the border boxes land where the arithmetic says: last row, last column, and a centre exactly on a cell border
    # belongs to the cell that starts there (offset 0)
    (H, W), (gh, gw), boxes, classes = next(iter(gen_inputs.nonsquare_encoder_cases()))
    lab = T.encode_boxes(boxes[0], classes[0], (H, W), (gh, gw), 4)
    assert lab[gh - 1, 2, 4] == 1 and lab[1, gw - 1, 4] == 1 and lab[gh - 1, gw - 1, 4] == 1
    assert lab[3, 4, 4] == 1 and lab[3, 4, 0] == 0 and lab[3, 4, 1] == 0
    assert lab[..., 4].sum() == len(boxes[0])


def test_evaluation_matches_reference_on_a_non_square_grid():
    y_true, lv0, lv1 = gen_inputs.nonsquare_measurement_inputs()
    assert y_true.shape[1:3] == (6, 10) and lv0.shape[1:3] == (6, 10) and lv1.shape[1:3] == (3, 5)
    kw = dict(gen_inputs.NONSQUARE_SCORE_KW)
    pm = kw.pop("precision_mode")
    counts = OMS.score_counts(y_true, (lv0, lv1), 3, version=3, **kw)
    p, r, f1 = OMS.score_table(counts, pm)
    eq = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)
    assert eq(p, G["score_precision"]) and eq(r, G["score_recall"]) and eq(f1, G["score_F1-score"])
    assert np.array_equal(counts[:, 1], G["score_gts"]) and np.array_equal(counts[:, 0], G["score_dets"])
    ps, rs = OMS.pr_curves(y_true, (lv0, lv1), 3, version=3, **gen_inputs.NONSQUARE_PR_KW)
    for c in range(3):
        assert eq(ps[c], G[f"pr_prec{c}"]) and eq(rs[c], G[f"pr_rec{c}"]) and len(ps[c]) > 3
    for mode in ("voc2007", "voc2012", "area", "smootharea"):
        assert eq(OMS.average_precisions(ps, rs, mode), G[f"pr_map_{mode}"])
