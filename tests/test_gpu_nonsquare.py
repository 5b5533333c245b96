"""Grids with gh != gw on the device: everything that knows about a grid -- the fused loss and its gradient, the metrics,
the loss-side IoU, decode / NMS, the label encoder and pyramid, the evaluation path -- on inputs for which
tests/test_nonsquare_cpu.py has shown that exchanging height and width gives visibly different results.
Loss / metrics / IoU against the float64 oracle at the tolerances of tests/test_gpu_loss.py and
tests/test_gpu_keras_shell.py; decode / NMS / labels / evaluation bit for bit against what the reference's own NumPy code
gave (tests/golden/nonsquare_golden.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_inputs  # noqa: E402
import nonsquare_cases as NS  # noqa: E402
from test_gpu_loss import check  # noqa: E402

from oracle import losses as OL  # noqa: E402
from oracle import tools as T  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "nonsquare_golden.npz"))
CASES = list(gen_inputs.nonsquare_decode_cases())


@pytest.mark.parametrize("case", NS.LOSS_CASES, ids=[c["id"] for c in NS.LOSS_CASES])
def test_loss_and_gradient(case):
    yt, yp = NS.build(case)
    check(NS.oracle_loss(case), NS.gpu_cfg(case), yt, yp)


@pytest.mark.parametrize("case", NS.METRIC_CASES, ids=[c["id"] for c in NS.METRIC_CASES])
def test_metrics(case):
    from tf2_yolo_amd import ops
    yt, yp = NS.build(case)
    (gh, gw), N, A = case["grid"], case["N"], case["A"]
    cfg = ops.make_loss_cfg(case["version"], N, gh, gw, A, case["C"], case["anchors"])
    out = ops.metrics(cfg, torch.tensor(yt).cuda(), torch.tensor(yp).cuda(), recall_thresh=0.5).cpu().numpy()
    ref = NS.oracle_metrics(case, yt, yp, 0.5)
    cells = N * gh * gw
    cls_den = out[2] if case["version"] == 1 else out[2] * A
    got = [out[0] / cells, out[1] / (out[2] + 1e-7), out[3] / (cls_den + 1e-7), out[4] / (out[2] + 1e-7)]
    print("metrics", case["id"], got, ref)
    assert out[5] == cells
    for a, b in zip(got, ref):
        assert abs(a - b) < 1e-5, (got, ref)


@pytest.mark.parametrize("grid,ciou", NS.IOU_CASES, ids=[f"{g[0]}x{g[1]}-{'ciou' if c else 'iou'}" for g, c in NS.IOU_CASES])
def test_loss_side_cal_iou(grid, ciou):
    """tf2_yolo_amd.losses.cal_iou_v4 / cal_iou_v3 (what yolovN.losses.cal_iou is) hand grid_shape[::-1] to the kernel"""
    from tf2_yolo_amd import losses
    t, p = NS.iou_operands(grid)
    t64, p64 = torch.tensor(t, dtype=torch.float64), torch.tensor(p, dtype=torch.float64)
    if ciou:
        iou, c = losses.cal_iou_v4(t, p, grid, return_ciou=True)
        ri, rc = OL.cal_iou(t64, p64, grid, return_ciou=True)
        assert np.abs(c.cpu().numpy() - rc.numpy()).max() <= 1e-6
    else:
        iou, ri = losses.cal_iou_v3(t, p, grid), OL.cal_iou(t64, p64, grid)
    assert iou.shape == (*t.shape[:3], p.shape[3]) and iou.dtype == torch.float32
    assert np.abs(iou.cpu().numpy() - ri.numpy()).max() <= 1e-6
    # the sliced view the losses pass
    yp = torch.tensor(np.concatenate([p, p[..., :1]], axis=-1)).cuda()
    v = losses.cal_iou_v4(t, yp[..., :4], grid, return_ciou=ciou)
    v = v[0] if isinstance(v, tuple) else v
    assert np.abs(v.cpu().numpy() - ri.numpy()).max() <= 1e-6


@pytest.mark.parametrize("walk", [0, 1], ids=["bit-matrix", "walk"])
@pytest.mark.parametrize("key,C,thr,lv", CASES, ids=[c[0] for c in CASES])
def test_decode_and_nms_golden(key, C, thr, lv, walk):
    """the bit-matrix NMS (default) and the greedy walk kernel (yolo_set_option(7, 1)), as
    tests/test_gpu_decode_nms.py::test_nms_bit_matrix_and_walk_give_the_same_rows selects them"""
    from tf2_yolo_amd import ops, tools
    try:
        ops.set_option(ops.OPT_NMS_WALK, walk)
        dec = tools.decode(*lv, class_num=C, threshold=thr, version=3)
        assert np.array_equal(dec.reshape(-1, 7), G[f"{key}_decode"])
        assert np.array_equal(tools.nms(dec, class_num=C, nms_threshold=0.5), G[f"{key}_nms"])
        assert np.array_equal(tools.nms(dec, class_num=C, nms_threshold=0.5, iou_mode=2), G[f"{key}_diou"])
        assert np.array_equal(tools.soft_nms(dec, class_num=C, nms_threshold=0.5, conf_threshold=thr, sigma=0.5), G[f"{key}_soft"])
    finally:
        ops.reset_options()


def test_decode_v1_v2_and_float64_labels_golden():
    from tf2_yolo_amd import tools
    m = gen_inputs.nonsquare_misc_inputs()
    assert np.array_equal(tools.decode(m["v1_lv"], class_num=4, threshold=0.4, version=1), G["v1_decode"])
    assert np.array_equal(tools.decode(m["v2_lv"], class_num=20, threshold=0.8, version=2), G["v2_decode"])
    assert np.array_equal(tools.decode(m["label12x20"][0], class_num=3, threshold=0.5, version=3), G["label12x20_decode"])


def test_down2xlabel_and_class_weights_golden():
    from tf2_yolo_amd import ops
    from utils.tools import get_class_weight
    lab = gen_inputs.nonsquare_misc_inputs()["label12x20"]
    d64, d32 = ops.down2xlabel(torch.from_numpy(np.ascontiguousarray(lab)).cuda())
    assert tuple(d64.shape) == (2, 6, 10, 8)
    assert np.array_equal(d64.cpu().numpy(), G["label6x10"]) and np.array_equal(d32.cpu().numpy(), G["label6x10"].astype(np.float32))
    e64, e32 = ops.down2xlabel(d64)
    assert tuple(e64.shape) == (2, 3, 5, 8)
    assert np.array_equal(e64.cpu().numpy(), G["label3x5"]) and np.array_equal(e32.cpu().numpy(), G["label3x5"].astype(np.float32))
    assert np.array_equal(get_class_weight(lab[..., 4:5], "binary"), G["binary_weight"])
    for meth in ("alpha", "log", "effective"):
        assert np.array_equal(get_class_weight(lab[..., 5:], meth), G[f"class_weight_{meth}"])


def test_encoder_and_pyramid_match_the_oracle_bit_for_bit():
    """yolo_encode_labels (through labels.label_pyramid_device) on a 240 x 400 image / 6 x 10 grid and on the exchanged
    pair: boxes on the last row, the last column and exactly on a cell border"""
    from tf2_yolo_amd import labels
    C = 4
    for hw, grid, boxes, classes in gen_inputs.nonsquare_encoder_cases():
        got = labels.label_pyramid_device(boxes, classes, hw, grid, C, 2)
        fine = np.stack([T.encode_boxes(b, c, hw, grid, C) for b, c in zip(boxes, classes)])
        ref = [T.down2xlabel(fine), fine]
        assert [tuple(g.shape) for g in got] == [(3, grid[0] // 2, grid[1] // 2, 5 + C), (3, grid[0], grid[1], 5 + C)]
        for g, r in zip(got, ref):
            assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), r.astype(np.float32))
        assert fine[0, ..., 4].sum() == len(boxes[0]) and fine[2].sum() == 0


def test_evaluation_golden():
    from utils.measurement import PRfunc, create_score_mat
    names = ["a", "b", "c"]
    y_true, lv0, lv1 = gen_inputs.nonsquare_measurement_inputs()
    eq = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)
    t = create_score_mat(y_true, lv0, lv1, class_names=names, version=3, **gen_inputs.NONSQUARE_SCORE_KW)
    for col in ("precision", "recall", "F1-score", "gts", "dets"):
        assert eq(t[col].to_numpy(), G[f"score_{col}"]), col
    f = PRfunc(y_true, lv0, lv1, class_names=names, version=3, **gen_inputs.NONSQUARE_PR_KW)
    for c in range(3):
        assert eq(f.precisions[c], G[f"pr_prec{c}"]) and eq(f.recalls[c], G[f"pr_rec{c}"]), c
    for mode in ("voc2007", "voc2012", "area", "smootharea"):
        assert eq(f.get_map(mode)["ap"].to_numpy(), G[f"pr_map_{mode}"]), mode


def test_train_steps_on_a_non_square_input_first_step_equals_the_oracle():
    """compile / train_on_batch on YOLOv3 64 x 96 with yolo.loss() and yolo.metrics("obj+iou+class+recall0.5"): the per-level
    grids the facade derives (grid_shape[0] * amp, grid_shape[1] * amp) reach the loss and the metric closures the right way
    round. The first step's loss and its four metrics per level equal the float64 oracle's on the same batch -- evaluated on
    the predictions of the device's own training-mode forward with the initial weights, so this compares the loss / metric
    plumbing (1e-5, as tests/test_gpu_keras_shell.py::test_readme_flow_v3 and test_gpu_loss.py::test_metrics), not
    the network's arithmetic, which test_gpu_model.py::test_model_parity[3-True-64x96] covers."""
    from yolov3 import Yolo
    from oracle import metrics as OM
    from tf2_yolo_amd import labels
    from tf2_yolo_amd.optimizers import Adam
    from test_gpu_model import A9
    H, W, C, N = 64, 96, 3, 4
    yolo = Yolo((H, W, 3), ["a", "b", "c"])
    yolo.create_model(anchors=A9, pretrained_body=None)
    assert tuple(yolo.grid_shape) == (2, 3)
    x, ys = labels.synthetic_batch(np.random.default_rng(8), N, (H, W), C)
    assert [y.shape[1:3] for y in ys] == [(2, 3), (4, 6), (8, 12)]
    yolo.model.compile(optimizer=Adam(learning_rate=1e-4), loss=yolo.loss(), metrics=yolo.metrics("obj+iou+class+recall0.5"))
    outs = [o.double().cpu() for o in yolo.model(x, training=True)]
    hist = [yolo.model.train_on_batch(x, ys) for _ in range(3)]
    assert all(len(h) == 1 + 3 + 12 and np.isfinite(h).all() for h in hist) and hist[1][0] != hist[0][0]
    ref_losses, ref_metrics = [], []
    for i, (o, yt) in enumerate(zip(outs, ys)):
        g = (2 * 2 ** i, 3 * 2 ** i)
        t = torch.tensor(yt, dtype=torch.float64)
        ref_losses.append(OL.wrap_yolo_loss_v3(g, 3, C, anchors=A9[3 * i:3 * i + 3], loss_weight=[1, 1, 5, 1])(t, o).item())
        ref_metrics += [OM.obj_acc(t, o, g, 3, C).mean().item(), OM.mean_iou(t, o, g, 3, C).item(),
                        OM.class_acc(t, o, g, 3, C).item(), OM.recall(t, o, g, 3, C, 0.5).item()]
    got = hist[0]
    print("first step", got, "oracle", sum(ref_losses), ref_losses, ref_metrics)
    assert abs(got[0] - sum(ref_losses)) <= 1e-5 * max(1.0, abs(sum(ref_losses)))
    for a, b in zip(got[1:4], ref_losses):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (got[1:4], ref_losses)
    for a, b in zip(got[4:], ref_metrics):
        assert abs(a - b) < 1e-5, (got[4:], ref_metrics)
