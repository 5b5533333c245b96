"""Half-precision inference, host side (no GPU): the precision string -> YOLO_PREC_* helper and the four
yolo_conv2d_fwd_*_ex entry points in the header, the ctypes table and the library."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = ["yolo_conv2d_fwd_planes_ex", "yolo_conv2d_fwd_planes_epi_ex", "yolo_conv2d_fwd_infer_unit_ex",
      "yolo_conv2d_fwd_head_unit_ex"]


def test_precision_helper_maps_the_two_names_and_rejects_the_rest():
    from tf2_yolo_amd import _lib, ops
    assert ops.precision_enum is _lib.precision_enum
    assert (_lib.PREC_F32, _lib.PREC_F16) == (0, 1)
    assert _lib.precision_enum("fp32") == _lib.PREC_F32 and _lib.precision_enum("fp16") == _lib.PREC_F16
    for bad in ("int8", "FP16", "bf16", "", None, 1, 0, ["fp16"]):
        with pytest.raises(ValueError, match="precision"):
            _lib.precision_enum(bad)


def test_header_declares_the_enum_and_the_four_entry_points():
    from tf2_yolo_amd import _lib
    src = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    assert re.search(r"enum\s*\{\s*YOLO_PREC_F32\s*=\s*0\s*,\s*YOLO_PREC_F16\s*=\s*1\s*\}", src)
    for name in EX:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        # the counterpart's arguments with `int precision` in front of the stream
        assert args[-2] == "int precision" and args[-1] == "void* stream", (name, args[-2:])
        old = re.search(r"\bint\s+" + name[:-3] + r"\s*\(([^;]*)\)\s*;", src)
        assert old and len(args) == len(old.group(1).split(",")) + 1, name
        res, argtypes = _lib.SIGNATURES[name]
        _, old_types = _lib.SIGNATURES[name[:-3]]
        assert res is ctypes.c_int and argtypes == old_types[:-1] + [ctypes.c_int, old_types[-1]], name


def test_library_exports_the_entry_points():
    from tf2_yolo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU
    for name in EX:
        assert hasattr(lib, name), name


def test_python_layers_take_a_named_precision_argument():
    """ops wrappers, Network.forward / infer and Model.predict: `precision` is a named parameter that defaults to fp32
    (predict swallows unknown keywords, so it must not arrive through **_); __call__ and evaluate do not have it"""
    from tf2_yolo_amd import ops
    from tf2_yolo_amd.engine import Network
    from tf2_yolo_amd.model import Model
    fns = [ops.conv2d_fwd_planes, ops.conv2d_fwd_planes_epi, ops.conv2d_fwd_infer_unit, ops.conv2d_fwd_head_unit,
           Network.forward, Network.infer, Model.predict]
    for f in fns:
        p = inspect.signature(f).parameters
        assert "precision" in p and p["precision"].default == "fp32", f.__qualname__
    for f in (Model.__call__, Model.evaluate):
        assert "precision" not in inspect.signature(f).parameters, f.__qualname__
