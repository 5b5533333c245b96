"""Loss / metrics / loss-side IoU cases on grids with gh != gw, shared by tests/test_nonsquare_cpu.py (which proves on the
float64 oracle that the inputs tell a height / width mix-up from the truth) and tests/test_gpu_nonsquare.py (which runs the
kernels on them).

The cell offsets x, y enter the losses only through the IoU, as x / gw and y / gh (oracle/losses.py:cal_iou), and in
YOLOv2 / v3 that IoU only takes decisions (responsible anchor, ignore mask). Uniform random predictions hardly ever sit
near one of those decisions, so `build` plants predictions that do (`_plant`): in every object cell box 0 is the true box
moved along x and box 1 the true box moved along y, by nearly the same fraction of the box; which of the two is the
responsible one depends on which of gh, gw divides which offset. Box 2 (where there is one) is moved along x by about a
third of the box, so that its IoU straddles the ignore threshold 0.6 and the recall threshold 0.5. Boxes 0 and 2 predict
the true class, box 1 guesses. Confidences follow the objects, so that obj_acc sees where the objects are."""
import numpy as np

from test_gpu_loss import ANCH9, make_case

A5 = [(0.04405615, 0.05210654), (0.14418923, 0.15865615), (0.25680231, 0.42110308), (0.60637077, 0.27136769),
      (0.75157846, 0.70525231)]
A4 = [[0.75493421, 0.65953947], [0.31578947, 0.39967105], [0.23355263, 0.18092105]]


def _case(name, version, grid, A, C, anchors, seed, N=3, obj_frac=0.35, r=0.12, **kw):
    """anchors: what the loss is given (None: YOLOv3 without anchors, and YOLOv1); r: how far boxes 0 and 1 are moved, as a
    fraction of the box"""
    return dict(id=name, version=version, grid=grid, N=N, A=A, C=C, anchors=anchors, seed=seed, obj_frac=obj_frac, r=r, kw=kw)


_W3 = dict(binary_weight=0.7, loss_weight=[1.5, 1.2, 5, 0.8], ignore_thresh=0.6)
_W4 = dict(binary_weight=0.9, loss_weight=[1, 5, 1], wh_reg_weight=0.01, ignore_thresh=0.6)
_W1 = dict(binary_weight=0.3, loss_weight=[5, 5, 1, 1])

# (kw holds the ORACLE's keyword names; `gpu_cfg` renames focal_loss_gamma for ops.make_loss_cfg)
LOSS_CASES = [
    _case("v3-3x7", 3, (3, 7), 3, 6, ANCH9[0:3], 101, use_focal_loss=False, use_scale=True, focal_loss_gamma=2, **_W3),
    _case("v3-7x3-focal", 3, (7, 3), 3, 6, ANCH9[3:6], 102, use_focal_loss=True, use_scale=True, focal_loss_gamma=2, **_W3),
    _case("v3-13x19-noscale", 3, (13, 19), 3, 6, ANCH9[6:9], 103, use_focal_loss=False, use_scale=False, focal_loss_gamma=2, **_W3),
    _case("v3-20x12-focal1.5-noscale", 3, (20, 12), 3, 6, ANCH9[0:3], 104, use_focal_loss=True, use_scale=False,
          focal_loss_gamma=1.5, **_W3),
    _case("v3-13x19-focal1.5", 3, (13, 19), 3, 6, ANCH9[3:6], 105, use_focal_loss=True, use_scale=True, focal_loss_gamma=1.5, **_W3),
    _case("v3-7x3-c80", 3, (7, 3), 3, 80, ANCH9[0:3], 106, loss_weight=[1, 1, 5, 1]),
    _case("v3-3x7-no-anchors", 3, (3, 7), 3, 6, None, 107),
    _case("v3-20x12-no-anchors", 3, (20, 12), 3, 6, None, 108),
    _case("v4-5x3", 4, (5, 3), 3, 5, A4, 141, N=2, truth_thresh=1.0, label_smooth=0.0, focal_loss_gamma=2, **_W4),
    _case("v4-3x5-truth0.7", 4, (3, 5), 3, 5, A4, 142, N=2, truth_thresh=0.7, label_smooth=0.0, focal_loss_gamma=2, **_W4),
    _case("v4-19x11-smooth0.1", 4, (19, 11), 3, 5, A4, 143, N=2, truth_thresh=1.0, label_smooth=0.1, focal_loss_gamma=2, **_W4),
    _case("v4-19x11-truth0.7-smooth0.05-gamma1.5", 4, (19, 11), 3, 5, A4, 144, N=2, truth_thresh=0.7, label_smooth=0.05,
          focal_loss_gamma=1.5, **_W4),
    _case("v4-5x3-truth0.7-smooth0.05", 4, (5, 3), 3, 5, A4, 145, N=2, truth_thresh=0.7, label_smooth=0.05, focal_loss_gamma=2, **_W4),
    _case("v2-13x9", 2, (13, 9), 5, 20, A5, 121, N=2, binary_weight=0.5, loss_weight=[1, 1, 5, 1], ignore_thresh=0.6),
    _case("v2-4x6", 2, (4, 6), 5, 20, A5, 122, N=2, binary_weight=0.5, loss_weight=[1, 1, 5, 1], ignore_thresh=0.6),
    _case("v1-4x7-c1", 1, (4, 7), 2, 1, None, 161, obj_frac=0.4, r=0.3, **_W1),
    _case("v1-7x4-c4", 1, (7, 4), 2, 4, None, 162, obj_frac=0.4, r=0.3, **_W1),
    _case("v1-4x7-c4", 1, (4, 7), 2, 4, None, 163, obj_frac=0.4, r=0.3, **_W1),
    _case("v1-7x4-c1", 1, (7, 4), 2, 1, None, 164, obj_frac=0.4, r=0.3, **_W1),
]

METRIC_CASES = [
    _case("v3-3x7", 3, (3, 7), 3, 6, ANCH9[0:3], 201, N=8, r=0.4),
    _case("v3-7x3", 3, (7, 3), 3, 6, ANCH9[0:3], 202, N=8, r=0.4),
    _case("v1-4x7", 1, (4, 7), 2, 5, None, 203, N=8, obj_frac=0.4, r=0.4),
    _case("v1-7x4", 1, (7, 4), 2, 5, None, 204, N=8, obj_frac=0.4, r=0.4),
]

IOU_CASES = [((5, 9), False), ((9, 5), False), ((5, 9), True), ((9, 5), True)]


def _plant(case, yt, yp):
    gh, gw = case["grid"]
    N, A, C, v1 = case["N"], case["A"], case["C"], case["version"] == 1
    rng = np.random.default_rng(case["seed"] + 5000)
    if v1:
        boxes = yp[..., :5 * A].reshape(N, gh, gw, A, 5)          # (views: the writes below land in yp)
        prob = None
    else:
        boxes = yp.reshape(N, gh, gw, A, 5 + C)
        prob = boxes[..., 5:]
    obj = yt[..., 4] > 0
    n = int(obj.sum())
    boxes[~obj, :, 4] *= 0.6                                       # background: mostly below 0.5
    t = yt[obj]                                                    # [n, 5 + C]
    tx, ty, tw, th = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    r = case["r"] * (0.7 + 0.6 * rng.random(n))
    # the box moved along the axis with the LARGER divisor is the closer one, by a hair, under the right divisors
    rx, ry = (0.9 * r, r) if gw > gh else (r, 0.9 * r)
    cell = boxes[obj]                                              # [n, A, 5(+C)] copy
    def moved(off, delta):
        return np.where(off < 0.5, off + delta, off - delta).astype(np.float32)
    dx = np.minimum(rx * gw * tw, 0.49)
    dy = np.minimum(ry * gh * th, 0.49)
    cell[:, 0, 0:4] = np.stack([moved(tx, dx), ty, tw, th], axis=1)
    cell[:, 1, 0:4] = np.stack([tx, moved(ty, dy), tw, th], axis=1)
    cell[:, 0:2, 4] = 0.55 + 0.4 * rng.random((n, 2))
    if prob is not None:                                           # box 0 knows the class, box 1 guesses
        cell[:, 0, 5:] = 0.01 + 0.1 * rng.random((n, C))
        cell[np.arange(n), 0, 5 + t[:, 5:].argmax(-1)] = 0.95
    if A >= 3:
        d2 = np.minimum(0.29 * (0.7 + 0.6 * rng.random(n)) * gw * tw, 0.49)
        cell[:, 2, 0:4] = np.stack([moved(tx, d2), ty, tw, th], axis=1)
        if prob is not None:
            cell[:, 2, 5:] = 0.01 + 0.4 * rng.random((n, C))
            cell[np.arange(n), 2, 5 + t[:, 5:].argmax(-1)] = 0.9
    boxes[obj] = cell
    if v1 and C > 1:                                               # YOLOv1: one class vector per cell; two in three know the class
        p = yp[obj, 5 * A:]
        know = rng.random(n) < 0.67
        p[know] *= 0.3
        p[know, t[know, 5:].argmax(-1)] += 0.7
        yp[obj, 5 * A:] = p
    if case["version"] == 2:                                       # softmax-normalised classes
        prob /= prob.sum(-1, keepdims=True)


def build(case):
    """-> y_true [N, gh, gw, 5 + C], y_pred [N, gh, gw, A (5 + C)] (version 1: [N, gh, gw, 5 A + C]), float32"""
    data_anchors = case["anchors"] if case["anchors"] is not None or case["version"] == 1 else ANCH9[0:3]
    yt, yp = make_case(case["N"], case["grid"], case["A"], case["C"], data_anchors, seed=case["seed"],
                       v1=case["version"] == 1, obj_frac=case["obj_frac"])
    yp = np.ascontiguousarray(yp)
    _plant(case, yt, yp)
    return yt, yp


def oracle_loss(case, grid=None):
    from oracle import losses as OL
    grid = tuple(grid or case["grid"])
    A, C, v = case["A"], case["C"], case["version"]
    if v == 3:
        return OL.wrap_yolo_loss_v3(grid, A, C, anchors=case["anchors"], **case["kw"])
    if v == 4:
        return OL.wrap_yolo_loss_v4(grid, A, C, case["anchors"], **case["kw"])
    if v == 2:
        return OL.wrap_yolo_loss_v2(grid, A, C, case["anchors"], **case["kw"])
    return OL.wrap_yolo_loss_v1(grid, A, C, **case["kw"])


def gpu_cfg(case):
    from tf2_yolo_amd import ops
    kw = dict(case["kw"])
    if "focal_loss_gamma" in kw:
        kw["focal_gamma"] = kw.pop("focal_loss_gamma")
    gh, gw = case["grid"]
    return ops.make_loss_cfg(case["version"], case["N"], gh, gw, case["A"], case["C"], case["anchors"], **kw)


def oracle_metrics(case, yt, yp, recall_thresh=0.5):
    """[obj_acc, mean_iou, class_acc, recall] of the float64 oracle (oracle/metrics.py)"""
    import torch
    from oracle import metrics as OM
    g, A, C = tuple(case["grid"]), case["A"], case["C"]
    t, p = torch.tensor(yt, dtype=torch.float64), torch.tensor(yp, dtype=torch.float64)
    if case["version"] == 1:
        return [OM.obj_acc_v1(t, p, g, A, C).mean().item(), OM.mean_iou_v1(t, p, g, A, C).item(),
                OM.class_acc_v1(t, p, g, C).item(), OM.recall_v1(t, p, g, A, C, recall_thresh).item()]
    return [OM.obj_acc(t, p, g, A, C).mean().item(), OM.mean_iou(t, p, g, A, C).item(),
            OM.class_acc(t, p, g, A, C).item(), OM.recall(t, p, g, A, C, recall_thresh).item()]


def iou_operands(grid, seed=7, N=2, B=3):
    """the losses' own call shape: (N, gh, gw, 1, 4) against (N, gh, gw, B, 4), as tests/test_gpu_keras_shell.py draws them"""
    gh, gw = grid
    rng = np.random.default_rng(seed + gh)
    t = rng.random((N, gh, gw, 1, 4)).astype(np.float32)
    p = rng.random((N, gh, gw, B, 4)).astype(np.float32)
    t[..., 2:] = t[..., 2:] * 0.5 + 0.05
    p[..., 2:] = p[..., 2:] * 0.5 + 0.05
    return t, p


def transpose_truth(yt):
    """the label tensor as a loader reads it that walks the cells column by column: cell (y, x) gets the label of the cell
    with the transposed flat index"""
    N, gh, gw, ch = yt.shape
    return np.ascontiguousarray(yt.transpose(0, 2, 1, 3)).reshape(N, gh, gw, ch)
