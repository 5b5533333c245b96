"""tools.detect_batch / Model.detect without a device: the argument errors are raised before anything touches the GPU, the
C entry points of the batched path are declared, exported and bound, and a valid call without a device fails loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_decode_batch_workspace_bytes", "yolo_decode_batch_count", "yolo_decode_batch_write",
               "yolo_nms_batch_workspace_bytes", "yolo_nms_batch_prepare", "yolo_nms_batch_select")


def _levels(B=2):
    return [np.zeros((B, 2, 2, 3 * 8), dtype=np.float32), np.zeros((B, 4, 4, 3 * 8), dtype=np.float32)]


@pytest.fixture
def no_device(monkeypatch):
    """any touch of the device after the argument checks would be a YoloHipError, with or without a GPU in the box"""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_argument_errors_come_before_the_device(no_device):
    from tf2_yolo_amd import tools
    with pytest.raises(ValueError, match="Invalid version"):
        tools.detect_batch(*_levels(), class_num=3, version=5)
    with pytest.raises(ValueError, match="nms_mode"):
        tools.detect_batch(*_levels(), class_num=3, nms_mode=4)
    with pytest.raises(ValueError, match="batch sizes"):
        tools.detect_batch(_levels(2)[0], _levels(3)[1], class_num=3)
    with pytest.raises(ValueError, match="shape"):
        tools.detect_batch(_levels()[0], _levels()[1][0], class_num=3)          # a level without its batch axis
    with pytest.raises(ValueError, match="shape"):
        tools.detect_batch_device(np.zeros((2, 2, 2, 2, 24), dtype=np.float32), class_num=3)


def test_valid_call_without_a_device_is_an_error(no_device):
    from tf2_yolo_amd import tools
    from tf2_yolo_amd._lib import YoloHipError
    with pytest.raises(YoloHipError):
        tools.detect_batch(*_levels(), class_num=3, nms_mode=1)


def test_reference_module_exports_detect_batch():
    import utils.tools
    from tf2_yolo_amd import tools
    assert utils.tools.detect_batch is tools.detect_batch
    assert utils.tools.decode is tools.decode and utils.tools.nms is tools.nms      # its neighbours are where they were


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
    # the size queries answer on the host and never land on a launch tape
    assert {"yolo_decode_batch_workspace_bytes", "yolo_nms_batch_workspace_bytes"} <= _lib._QUERIES


def test_workspace_queries():
    """decode: one int per workgroup of 2 048 candidates and image, plus one; NMS: no room for bit matrices (the batched path
    sizes them from the segment counts), so far below the per-image bound for the same rows"""
    from tf2_yolo_amd import _lib
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    q = lib.yolo_decode_batch_workspace_bytes
    assert q(3, ints(13, 26, 52), ints(13, 26, 52), ints(3, 3, 3), 80, 32) == ((20 + 80 + 317) * 32 + 1) * 4
    assert q(1, ints(2), ints(3), ints(3), 5, 4) == (1 * 4 + 1) * 4
    assert q(0, ints(2), ints(3), ints(3), 5, 4) == 0 and q(9, ints(*[2] * 9), ints(*[2] * 9), ints(*[3] * 9), 5, 4) == 0
    assert q(1, ints(0), ints(3), ints(3), 5, 4) == 0
    n, B, C = 1_500_000, 32, 80
    batch, single = lib.yolo_nms_batch_workspace_bytes(n, B, C), lib.yolo_nms_workspace_bytes(n, C)
    assert single > 1_500_000_000 and 0 < batch < 150_000_000
    assert lib.yolo_nms_batch_workspace_bytes(0, B, C) == 256


def test_entry_points_validate_before_launching():
    """bad arguments are YOLO_ERR_INVALID_ARG (-1) with a message, a short workspace is YOLO_ERR_WORKSPACE (-3), without a device"""
    from tf2_yolo_amd import _lib
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    one = ctypes.c_void_p(8)          # never dereferenced: the checks below fail first
    preds = (ctypes.c_void_p * 1)(8)
    thr = (ctypes.c_double * 1)(0.5)
    assert lib.yolo_decode_batch_count(preds, ints(0), 1, 2, ints(2), ints(2), ints(3), 5, 7, thr, one, one, 1 << 20, None) == -1
    assert b"Invalid version: 7" in lib.yolo_last_error()
    assert lib.yolo_decode_batch_count(preds, ints(0), 9, 2, ints(2), ints(2), ints(3), 5, 3, thr, one, one, 1 << 20, None) == -1
    assert lib.yolo_decode_batch_write(preds, ints(0), 1, 2, ints(2), ints(2), ints(3), 5, 3, thr, None, 4, one, 1 << 20,
                                       None) == -1
    assert lib.yolo_decode_batch_count(preds, ints(0), 1, 2, ints(2), ints(2), ints(3), 5, 3, thr, one, one, 4, None) == -3
    assert b"workspace" in lib.yolo_last_error()
    assert lib.yolo_nms_batch_prepare(one, 5, one, 0, 3, one, one, 1 << 20, None) == -1
    assert lib.yolo_nms_batch_prepare(one, 5, one, 2, 3, one, one, 16, None) == -3
    assert b"workspace" in lib.yolo_last_error()
    assert lib.yolo_nms_batch_select(one, 5, 2, 3, 9, 0.45, 0.5, 0.5, None, 0, one, one, one, one, 1 << 20, None) == -1
    assert b"bad mode 9" in lib.yolo_last_error()
    assert lib.yolo_nms_batch_select(one, 5, 2, 3, 1, 0.45, 0.5, 0.5, None, 7, one, one, one, one, 1 << 20, None) == -1


def test_model_detect_argument_errors_need_no_device():
    """Model.detect's own checks (nms_mode, precision, a classifier) are covered on the GPU (tests/test_gpu_detect_batch.py):
    a Model cannot be built without one. Here: the method exists with the signature the documents give."""
    import inspect
    from tf2_yolo_amd.model import Model
    sig = inspect.signature(Model.detect)
    assert list(sig.parameters) == ["self", "x", "batch_size", "precision", "conf_threshold", "nms_mode", "nms_threshold",
                                    "nms_sigma"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["batch_size"], d["precision"], d["conf_threshold"], d["nms_mode"], d["nms_threshold"], d["nms_sigma"]) == \
        (32, "fp32", 0.5, 1, 0.45, 0.5)
    from tf2_yolo_amd import tools
    sig = inspect.signature(tools.detect_batch)
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(class_num=1, conf_threshold=0.5, nms_mode=0, nms_threshold=0.45, nms_sigma=0.5, version=3)
