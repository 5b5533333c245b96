"""Drop-in for the reference's utils/measurement.py (create_score_mat :16-150, PRfunc :153-447), on the GPU.

Same names, arguments, defaults and return types (pandas DataFrames; PRfunc.precisions / .recalls lists of
float64 arrays). The pipeline is decode -> NMS -> IoU matching -> per-image cap, for a chunk of images at a time and
all in HIP kernels (decode_nms.hip, measure.hip); the precision / recall curves of all classes are one more call over
the detections of the whole data set. `Evaluator` is that pipeline as an accumulator (update per chunk, score_mat /
prfunc at the end; Model.evaluate_detections feeds it the head buffers in place); create_score_mat and PRfunc cut their
arrays into chunks of EVAL_CHUNK images and feed one. Nothing is launched or read back per image or per class.

Differences, all in corners the reference leaves undefined or broken:
  * exact ties of the joint confidence: the later detection sorts first (np.argsort is unstable), in the per-image
    `max_per_img` cut and on the curve. "Later" is the row order of decode / NMS inside an image, then the image order.
    The order is total (measure.hip, yolo_rank_desc): -0.0 and 0.0 tie, and a NaN confidence would order as +inf, i.e.
    first, like the reference's argsort()[::-1] -- decode never lets one through (`conf * prob >= threshold` is false);
  * a class without any detection: the reference re-uses `num_tp` of the PREVIOUS class (or raises
    NameError for class 0); here its curve is the single point (0, 0) -- (0, nan) if it also has no
    ground truth;
  * a class with detections but no ground truth: the reference divides by zero (ZeroDivisionError); here
    recall is nan and precision follows the formulas with num_tp = 0.
"""
import warnings

import numpy as np
import torch

from . import ops, tools
from ._lib import YoloHipError


EVAL_CHUNK = 256   # images per Evaluator.update of create_score_mat / PRfunc (at 416 x 416 and C = 80: ~0.9 GB of fp32 levels)


def _shape(a):
    return tuple(a.shape) if torch.is_tensor(a) else np.shape(a)


class Evaluator(object):
    """Detection evaluation of a data set, chunk by chunk, on the device: update(y_true, *y_preds) per chunk of images,
    then score_mat() (create_score_mat's table) and prfunc() (a PRfunc). The host reads a fixed number of scalars and
    offsets per chunk (decode_batch, nms_batch_select), whatever the number of images and classes; the per-class counts
    and the records of the kept detections (joint confidence, ground-truth id, matched, class) stay on the device.

    Per chunk: ground truth through ops.decode_batch (threshold 0.5), detections through tools._detect_batch_flat
    (decode + NMS), ops.match_batch, the cap of max_per_img detections per image and class (ops.rank_desc_images; None:
    no cap), and the records are appended. Image b of a chunk is evaluated as create_score_mat / PRfunc evaluate it, bit
    for bit; the chunking does not enter the result. class_names=[]: nothing to evaluate, empty tables and curves."""

    def __init__(self, class_names, version=3, conf_threshold=0.05, nms_mode=1, nms_threshold=0.5, nms_sigma=0.5,
                 iou_threshold=0.5, precision_mode=2, max_per_img=100):
        if version not in (1, 2, 3, 4):
            raise ValueError(f"Invalid version: {version}")
        if nms_mode not in (0, 1, 2, 3):
            raise ValueError(f"Invalid nms_mode: {nms_mode} (0: none, 1: NMS, 2: soft-NMS, 3: DIoU-NMS)")
        self.class_names = class_names
        self.class_num = len(class_names)
        self.version = version
        self.conf_threshold, self.nms_mode, self.nms_threshold, self.nms_sigma = conf_threshold, nms_mode, nms_threshold, nms_sigma
        self.iou_threshold, self.precision_mode, self.max_per_img = iou_threshold, precision_mode, max_per_img
        self.images = 0
        self._gts = self._counts = None       # int64 [C] / [C, 4] on the device, made by the first update
        self._gt_rows = 0                     # decoded ground-truth rows so far: a host-side bound of gts.sum()
        self._records = []                    # per chunk: (joint, gid, matched, cls), cls = -1 where the row is cut

    def update(self, y_true, *y_preds):
        """one chunk: y_true [B, gh, gw, info], every prediction level [B, ...]; NumPy arrays are uploaded, CUDA tensors are
        used in place (they are free again when update returns)"""
        self._update(y_true, y_preds, True)

    def _update(self, y_true, y_preds, records):
        B = tools._check_batch_args(y_preds, self.nms_mode, self.version)
        s = _shape(y_true)
        if len(s) != 4:
            raise ValueError(f"y_true must have shape (batch, grid_heights, grid_widths, info), got {s}")
        if s[0] != B:
            raise ValueError(f"y_true and the prediction levels hold different batch sizes: {s[0]} and {B}")
        dev = tools._device()
        C = self.class_num
        self.images += B
        if C == 0 or B == 0:
            return
        if self._gts is None:
            self._gts = torch.zeros(C, device=dev, dtype=torch.int64)
            self._counts = torch.zeros((C, 4), device=dev, dtype=torch.int64)   # dets, gts, tpp, tp
        y_true = tools._to_dev(y_true)
        anchors = (s[3] - C) // 5 if self.version == 1 else s[3] // (5 + C)
        gt, gt_off = ops.decode_batch([y_true], [anchors], C, self.version, [0.5])
        det, offs = tools._detect_batch_flat(y_preds, C, self.conf_threshold, self.nms_mode, self.nms_threshold,
                                             self.nms_sigma, self.version)
        det_off = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int32)).to(dev)
        _, matched, _, gid = ops.match_batch(gt, gt_off, det, det_off, C, self.iou_threshold, self._gts, self._counts)
        self._gt_rows += int(gt.shape[0])
        if not records or det.shape[0] == 0:
            return
        cls = det[:, 5].to(torch.int32)
        joint = (det[:, 4] * det[:, 6]).contiguous()
        keep = (cls >= 0) & (cls < C)
        if self.max_per_img is not None:
            keep &= ops.rank_desc_images(joint, cls, det_off) < self.max_per_img
        # (no compaction, which would be a host read: ops.pr_curves passes over the rows of class -1)
        self._records.append((joint, gid, matched, torch.where(keep, cls, torch.full_like(cls, -1))))

    def score_mat(self, precision_mode=None):
        """create_score_mat's table of what update has seen (precision_mode None: the constructor's)"""
        import pandas as pd
        precision_mode = self.precision_mode if precision_mode is None else precision_mode
        class_num = self.class_num
        if self._counts is None:
            c = np.zeros((class_num, 4))
        else:
            c = self._counts.cpu().numpy().astype(np.float64)   # dets, gts, tpp, tp
        dets, gts, tpp, tp = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        denom_p = dets - (tpp - tp) if precision_mode == 1 else dets
        num_p = tpp if precision_mode == 0 else tp
        with np.errstate(divide="ignore", invalid="ignore"):
            precision = np.true_divide(num_p, denom_p)
            recall = np.true_divide(tp, gts)
            f1 = (2 * precision * recall) / (precision + recall)
        table = pd.DataFrame({"precision": precision, "recall": recall, "F1-score": f1,
                              "gts": gts.astype("int"), "dets": dets.astype("int")})
        table.index = self.class_names
        return table

    def _curves(self):
        """(precisions, recalls): one float64 array per class, from one ops.pr_curves call"""
        class_num = self.class_num
        n_c = np.zeros(class_num + 1, dtype=np.int64)
        gts_h = np.zeros(class_num, dtype=np.int64)
        if self._gts is not None:
            gts_h = self._gts.cpu().numpy()
        if self._records:
            joint, gid, matched, cls = (torch.cat(col) for col in zip(*self._records))
            cls_off, prec, rec = ops.pr_curves(joint, gid, matched, cls, self._gts, self.precision_mode,
                                               gts_total=self._gt_rows)
            off = cls_off.cpu().numpy().astype(np.int64)
            prec, rec = prec.cpu().numpy(), rec.cpu().numpy()
            n_c = np.diff(off)
        precisions, recalls = [], []
        for c in range(class_num):
            n, num_gts = int(n_c[c]), int(gts_h[c])
            if n == 0:
                precisions.append(np.array([0.0]))
                recalls.append(np.array([0.0 if num_gts > 0 else np.nan]))
            elif num_gts == 0:   # every detection is a false positive; recall undefined
                precisions.append(np.zeros(n + 1))
                recalls.append(np.full(n + 1, np.nan))
            else:
                first = int(off[c]) + c
                precisions.append(prec[first:first + n + 1].copy())
                recalls.append(rec[first:first + n + 1].copy())
        return precisions, recalls

    def prfunc(self):
        """the PRfunc of what update has seen: __call__, plot_pr_curve and get_map as ever"""
        f = PRfunc.__new__(PRfunc)
        f.class_num, f.class_names = self.class_num, self.class_names
        f.precisions, f.recalls = self._curves()
        return f


def _feed(ev, y_trues, y_preds, records):
    """the arrays of a data set through ev in chunks of EVAL_CHUNK images"""
    arrays = [a if torch.is_tensor(a) or isinstance(a, np.ndarray) else np.asarray(a) for a in (y_trues,) + tuple(y_preds)]
    for i in range(0, len(arrays[0]), EVAL_CHUNK):
        ev._update(arrays[0][i:i + EVAL_CHUNK], [a[i:i + EVAL_CHUNK] for a in arrays[1:]], records)
    return ev


def create_score_mat(y_trues, *y_preds, class_names=[], conf_threshold=0.5, nms_mode=0, nms_threshold=0.5,
                     nms_sigma=0.5, iou_threshold=0.5, precision_mode=2, version=3):
    """Score table (pandas.DataFrame: precision, recall, F1-score, gts, dets per class)."""
    if not torch.cuda.is_available():
        raise YoloHipError("tf2_yolo_amd.measurement needs a HIP device: there is no CPU fallback")
    ev = Evaluator(class_names, version=version, conf_threshold=conf_threshold, nms_mode=nms_mode, nms_threshold=nms_threshold,
                   nms_sigma=nms_sigma, iou_threshold=iou_threshold, precision_mode=precision_mode, max_per_img=None)
    return _feed(ev, y_trues, y_preds, False).score_mat()


class PRfunc(object):
    """Precision-recall function: call with a recall value (and class index) to get a precision value."""

    def __init__(self, y_trues, *y_preds, class_names=[], conf_threshold=0.05, nms_mode=1, nms_threshold=0.5,
                 nms_sigma=0.5, iou_threshold=0.5, precision_mode=2, max_per_img=100, version=3):
        if not torch.cuda.is_available():
            raise YoloHipError("tf2_yolo_amd.measurement needs a HIP device: there is no CPU fallback")
        ev = Evaluator(class_names, version=version, conf_threshold=conf_threshold, nms_mode=nms_mode,
                       nms_threshold=nms_threshold, nms_sigma=nms_sigma, iou_threshold=iou_threshold,
                       precision_mode=precision_mode, max_per_img=max_per_img)
        self.class_num = ev.class_num
        self.class_names = class_names
        self.precisions, self.recalls = _feed(ev, y_trues, y_preds, True)._curves()

    def __call__(self, recall, class_idx=0):
        if class_idx >= self.class_num:
            raise IndexError("Class index out of range")
        precisions = self.precisions[class_idx]
        recalls = self.recalls[class_idx]
        pc_idx = (recalls > recall).sum()
        if pc_idx == 0:
            return 0
        return precisions[-pc_idx:].max()

    def plot_pr_curve(self, class_idx=-1, smooth=False, figsize=None, return_fig=False):
        """Plot PR curve(s) with matplotlib (class_idx = -1: all classes; smooth: interpolated precision)."""
        import matplotlib.pyplot as plt
        if class_idx >= self.class_num:
            raise IndexError("Class index out of range")
        sl = slice(class_idx, class_idx + 1) if class_idx >= 0 else slice(None)
        fig = plt.figure(figsize=figsize)
        for precision, recall in zip(self.precisions[sl], self.recalls[sl]):
            if smooth:
                precision = np.maximum.accumulate(precision[::-1])[::-1]
            plt.plot(recall, precision)
        plt.legend(self.class_names[sl])
        plt.title("PR curve")
        plt.xlabel("recall")
        plt.ylabel("precision")
        plt.xlim(-0.05, 1.05)
        plt.ylim(-0.05, 1.05)
        if return_fig:
            return fig
        plt.show()

    def get_map(self, mode="voc2012"):
        """mAP table (pandas.DataFrame); mode in "voc2007", "voc2012", "area", "smootharea"."""
        import pandas as pd
        aps = [0 for _ in range(self.class_num)]
        if mode in ("area", "smootharea"):
            for c in range(self.class_num):
                precisions = self.precisions[c]
                if mode == "smootharea":
                    precisions = np.maximum.accumulate(precisions[::-1])[::-1]
                recalls = self.recalls[c]
                for i in range(len(precisions) - 1):   # trapezoids, summed left to right like the reference
                    aps[c] += (recalls[i + 1] - recalls[i]) * ((precisions[i + 1] - precisions[i]) / 2 + precisions[i])
        else:
            if mode == "voc2012":
                recall_list = [0, 0.14, 0.29, 0.43, 0.57, 0.71, 1]
            elif mode == "voc2007":
                recall_list = [i / 10 for i in range(0, 11)]
            else:
                raise ValueError(f"Invalid mode: {mode}")
            for c in range(self.class_num):
                for rc in recall_list:
                    aps[c] += self(rc, c)
            aps = [ap / len(recall_list) for ap in aps]
        aps.append(sum(aps) / len(aps))
        table = pd.DataFrame(aps)
        table.columns = ["ap"]
        table.index = list(self.class_names) + ["mAP"]
        return table


class PR_func(PRfunc):
    def __init__(self, *args, **kwargs):
        warnings.warn("`PR_func` is deprecated and renamed to `PRfunc`.", Warning)
        super().__init__(*args, **kwargs)
