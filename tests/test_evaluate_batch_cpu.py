"""Data-set evaluation on the device (measurement.Evaluator, Model.evaluate_detections, csrc/measure.hip) without a
device: the C entry points are declared, exported and bound, their size queries answer on the host, bad arguments and a
short workspace are refused before any launch, and the Python argument errors come before anything touches the GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_match_batch_workspace_bytes", "yolo_match_batch", "yolo_rank_desc_images",
               "yolo_pr_curves_workspace_bytes", "yolo_pr_curves")
QUERIES = {"yolo_match_batch_workspace_bytes", "yolo_pr_curves_workspace_bytes"}


@pytest.fixture
def no_device(monkeypatch):
    """any touch of the device after the argument checks would be a YoloHipError, with or without a GPU in the box"""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def _chunk(B=2, C=3):
    y_true = np.zeros((B, 4, 4, 5 + C))
    return y_true, np.zeros((B, 2, 2, 3 * (5 + C)), dtype=np.float32), np.zeros((B, 4, 4, 3 * (5 + C)), dtype=np.float32)


def test_new_entry_points_are_declared_exported_and_bound():
    from tf2_yolo_amd import _lib
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.yolo_abi_version() == 5          # additions only: the version stays
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/yolo_hip.h"
        assert hasattr(lib, name), f"libyolo_hip.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert QUERIES <= _lib._QUERIES               # the size queries never land on a launch tape
    for name in ("yolo_match_detections", "yolo_rank_desc", "yolo_pr_curve", "yolo_pr_curve_workspace_bytes"):
        assert hasattr(lib, name)                 # the single-image entry points stay exported


def test_shared_device_helpers_are_stated_once():
    """one evaluation source: iou_xywh is defined once under csrc/, in measure.hip, and desc_order_key once, in common.hpp"""
    csrc = os.path.join(ROOT, "tf2_yolo_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".hpp"))}
    for body, home in (("double iou_xywh(", "measure.hip"), ("double desc_order_key(", "common.hpp")):
        assert [n for n, s in src.items() if body in s] == [home]
    assert '#include "common.hpp"' in src["measure.hip"] and "desc_order_key(" in src["measure.hip"]
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(CSRC)/measure.hip" in make and "measure_batch" not in make


def test_workspace_queries():
    """match_batch: one flag byte per ground truth and 2 * B * C ints; pr_curves: per row one double, three ints and two
    bytes, one int per ground truth, per class an int and a long long; both in 256-byte pieces with 256 bytes to spare"""
    from tf2_yolo_amd import _lib
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    q = lib.yolo_match_batch_workspace_bytes
    assert q(1000, 4, 80) == up(2 * 4 * 80 * 4) + up(1000) + 256
    assert q(0, 1, 1) == up(8) + 256
    assert q(-1, 4, 80) == 256 and q(10, 0, 80) == 256 and q(10, 4, 0) == 256
    q = lib.yolo_pr_curves_workspace_bytes
    n, C, g = 3000, 80, 700
    assert q(n, C, g) == up(8 * n) + up(8 * (C + 1)) + up(4 * C) + 3 * up(4 * n) + up(4 * g) + 2 * up(n) + 256
    assert q(0, 1, 0) == up(16) + up(4) + 256
    assert q(-1, C, g) == 256 and q(n, 0, g) == 256 and q(n, C, -1) == 256


def test_entry_points_validate_before_launching():
    """bad arguments are YOLO_ERR_INVALID_ARG (-1) with a message, a short workspace is YOLO_ERR_WORKSPACE (-3), without a device"""
    from tf2_yolo_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)          # never dereferenced: the checks below fail first
    big = 1 << 20
    mb = lib.yolo_match_batch
    #        gt   ngt off  det ndet off  B  C  thr  seen best matched iou gid counts ws  bytes stream
    assert mb(one, 5, one, one, 7, one, 0, 3, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert b"match_batch: bad sizes" in lib.yolo_last_error()
    assert mb(one, -1, one, one, 7, one, 2, 3, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert mb(one, 5, one, one, -7, one, 2, 3, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert mb(one, 5, one, one, 7, one, 2, 0, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert mb(one, 5, one, one, 7, one, 2, 3, 0.5, None, one, one, one, one, one, one, big, None) == -1
    assert b"null pointer" in lib.yolo_last_error()
    assert mb(one, 5, None, one, 7, one, 2, 3, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert mb(one, 5, one, one, 7, one, 2, 3, 0.5, one, one, one, one, None, one, one, big, None) == -1      # no gid
    assert b"null detection buffers" in lib.yolo_last_error()
    assert mb(None, 5, one, one, 7, one, 2, 3, 0.5, one, one, one, one, one, one, one, big, None) == -1
    assert mb(one, 5, one, one, 7, one, 2, 3, 0.5, one, one, one, one, one, one, None, big, None) == -1
    need = lib.yolo_match_batch_workspace_bytes(5, 2, 3)
    assert mb(one, 5, one, one, 7, one, 2, 3, 0.5, one, one, one, one, one, one, one, need - 1, None) == -3
    assert b"workspace" in lib.yolo_last_error()

    rk = lib.yolo_rank_desc_images
    assert rk(one, one, -1, one, 2, one, None) == -1
    assert rk(one, one, 5, one, 0, one, None) == -1
    assert rk(None, one, 5, one, 2, one, None) == -1
    assert rk(one, one, 5, None, 2, one, None) == -1
    assert rk(one, None, 5, one, 2, None, None) == -1
    assert b"rank_desc_images: null pointer" in lib.yolo_last_error()
    assert rk(None, None, 0, None, 2, None, None) == 0          # nothing to rank, nothing launched

    pc = lib.yolo_pr_curves
    #        joint gid matched cls  n  gts  C  total mode ws  bytes off prec rec stream
    assert pc(one, one, one, one, 9, one, 4, 20, 3, one, big, one, one, one, None) == -1
    assert b"bad precision mode 3" in lib.yolo_last_error()
    assert pc(one, one, one, one, 9, one, 4, 20, -1, one, big, one, one, one, None) == -1
    assert pc(one, one, one, one, -9, one, 4, 20, 2, one, big, one, one, one, None) == -1
    assert b"pr_curves: bad sizes" in lib.yolo_last_error()
    assert pc(one, one, one, one, 9, one, 0, 20, 2, one, big, one, one, one, None) == -1
    assert pc(one, one, one, one, 9, one, 4, -1, 2, one, big, one, one, one, None) == -1
    assert pc(one, one, one, one, 9, None, 4, 20, 2, one, big, one, one, one, None) == -1
    assert pc(one, one, one, None, 9, one, 4, 20, 2, one, big, one, one, one, None) == -1
    assert pc(one, one, one, one, 9, one, 4, 20, 2, one, big, None, one, one, None) == -1
    assert pc(one, one, one, one, 9, one, 4, 20, 2, one, big, one, one, None, None) == -1
    assert b"null pointer" in lib.yolo_last_error()
    need = lib.yolo_pr_curves_workspace_bytes(9, 4, 20)
    assert pc(one, one, one, one, 9, one, 4, 20, 2, one, need - 1, one, one, one, None) == -3
    assert b"workspace" in lib.yolo_last_error()


def test_evaluator_argument_errors_come_before_the_device(no_device):
    from tf2_yolo_amd.measurement import Evaluator
    names = ["a", "b", "c"]
    with pytest.raises(ValueError, match="Invalid version"):
        Evaluator(names, version=5)
    with pytest.raises(ValueError, match="nms_mode"):
        Evaluator(names, nms_mode=4)
    y_true, lv0, lv1 = _chunk()
    ev = Evaluator(names)
    with pytest.raises(ValueError, match="shape"):
        ev.update(y_true, lv0, lv1[0])                     # a level without its batch axis
    with pytest.raises(ValueError, match="shape"):
        ev.update(y_true[0], lv0, lv1)                     # the labels without theirs
    with pytest.raises(ValueError, match="batch sizes"):
        ev.update(y_true, lv0, _chunk(3)[2])
    with pytest.raises(ValueError, match="batch sizes"):
        ev.update(_chunk(3)[0], lv0, lv1)
    with pytest.raises(ValueError, match="at least one level"):
        ev.update(y_true)
    assert ev.images == 0


def test_valid_update_without_a_device_is_an_error(no_device):
    from tf2_yolo_amd.measurement import Evaluator, PRfunc, create_score_mat
    from tf2_yolo_amd._lib import YoloHipError
    with pytest.raises(YoloHipError):
        Evaluator(["a", "b", "c"]).update(*_chunk())
    with pytest.raises(YoloHipError):
        Evaluator([]).update(*_chunk())
    with pytest.raises(YoloHipError):
        create_score_mat(*_chunk(), class_names=["a", "b", "c"])
    with pytest.raises(YoloHipError):
        PRfunc(*_chunk(), class_names=["a", "b", "c"])


def test_an_evaluator_that_saw_nothing(no_device):
    """no update, or no class: empty counts, the single-point curves of classes without detections -- and no device"""
    from tf2_yolo_amd.measurement import Evaluator, PRfunc
    ev = Evaluator(["a", "b"])
    t = ev.score_mat()
    assert list(t.index) == ["a", "b"] and list(t.columns) == ["precision", "recall", "F1-score", "gts", "dets"]
    assert (t["dets"].to_numpy() == 0).all() and np.isnan(t["precision"].to_numpy()).all()
    f = ev.prfunc()
    assert isinstance(f, PRfunc) and f.class_num == 2 and f.class_names == ["a", "b"]
    assert all(np.array_equal(p, [0.0]) for p in f.precisions) and all(np.isnan(r).all() and r.shape == (1,) for r in f.recalls)
    assert f(0.5, 1) == 0 and list(f.get_map("voc2007").index) == ["a", "b", "mAP"]
    none = Evaluator([])
    assert none.score_mat().shape == (0, 5) and none.prfunc().precisions == []


def test_signatures_and_defaults():
    from tf2_yolo_amd.measurement import EVAL_CHUNK, Evaluator
    from tf2_yolo_amd.model import Model
    sig = inspect.signature(Evaluator.__init__)
    assert list(sig.parameters) == ["self", "class_names", "version", "conf_threshold", "nms_mode", "nms_threshold", "nms_sigma",
                                    "iou_threshold", "precision_mode", "max_per_img"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(version=3, conf_threshold=0.05, nms_mode=1, nms_threshold=0.5, nms_sigma=0.5, iou_threshold=0.5,
                     precision_mode=2, max_per_img=100)
    sig = inspect.signature(Evaluator.update)
    assert [(p.name, p.kind) for p in sig.parameters.values()][1:] == [("y_true", inspect.Parameter.POSITIONAL_OR_KEYWORD),
                                                                       ("y_preds", inspect.Parameter.VAR_POSITIONAL)]
    assert inspect.signature(Evaluator.score_mat).parameters["precision_mode"].default is None
    assert list(inspect.signature(Evaluator.prfunc).parameters) == ["self"]
    sig = inspect.signature(Model.evaluate_detections)
    assert list(sig.parameters) == ["self", "x", "y", "class_names", "batch_size", "precision", "rescale", "conf_threshold",
                                    "nms_mode", "nms_threshold", "nms_sigma", "iou_threshold", "precision_mode", "max_per_img"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(batch_size=32, precision="fp32", rescale=None, conf_threshold=0.05, nms_mode=1, nms_threshold=0.5,
                     nms_sigma=0.5, iou_threshold=0.5, precision_mode=2, max_per_img=100)
    assert EVAL_CHUNK == 256
    from tf2_yolo_amd import ops
    for name in ("match_batch", "rank_desc_images", "pr_curves"):
        assert callable(getattr(ops, name))


def test_reference_module_exports_the_evaluator():
    import tf2_yolo_amd.measurement
    import utils.measurement
    assert utils.measurement.Evaluator is tf2_yolo_amd.measurement.Evaluator
    assert utils.measurement.PRfunc is tf2_yolo_amd.measurement.PRfunc          # its neighbours are where they were
    assert utils.measurement.create_score_mat is tf2_yolo_amd.measurement.create_score_mat


def test_drop_in_signatures_are_unchanged():
    from tf2_yolo_amd.measurement import PRfunc, create_score_mat
    d = {k: v.default for k, v in inspect.signature(create_score_mat).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(class_names=[], conf_threshold=0.5, nms_mode=0, nms_threshold=0.5, nms_sigma=0.5, iou_threshold=0.5,
                     precision_mode=2, version=3)
    d = {k: v.default for k, v in inspect.signature(PRfunc.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(class_names=[], conf_threshold=0.05, nms_mode=1, nms_threshold=0.5, nms_sigma=0.5, iou_threshold=0.5,
                     precision_mode=2, max_per_img=100, version=3)
