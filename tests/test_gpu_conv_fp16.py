"""Half-precision inference convolutions (include/yolo_hip.h: yolo_conv2d_fwd_*_ex with YOLO_PREC_F16): ONE fp16 MFMA pass
(h*h, csrc/planes.hpp) instead of three, in every kernel family the inference path reaches -- the per-tap streaming kernel
and its split-K form (conv_planes.hip), the window kernel with its patch, split-K and stream-K forms (conv_win.hip), the
few-output-pixel kernel and its head form (conv_small.hip) -- each forced the way tests/test_gpu_conv.py forces it.

Per case:
  exact   operands that fp16 holds exactly after the planes' scale (integers in [-8, 8] / 64: the l plane is zero): the fp16
          result is BIT-identical to the fp32-mode result of the same entry point (y, absmax, the infer unit's planes / words)
  arith   random operands (x ~ N(0, 1), He-scaled filters, seed 0): within 2e-5 of max|y| of the float64 convolution of the
          rounded operands hx = fp16(s_x x) / s_x, hw = fp16(s_w w) / s_w (the bar
          test_conv_planes_c3_layer_sizes_vs_fp64_oracle holds the three-pass kernels to), MORE than 1e-4 away from the
          float64 convolution of the unrounded ones (the feature is on: fp16 operand rounding is 2.3e-4 .. 4.0e-4 of max|y| on
          these shapes, computed on the CPU; three passes stay below 2e-5), and precision "fp32" through the _ex entry
          bit-identical to the entry point without the suffix.
The 1e-4 distance is asserted where the output IS the convolution (plain entry, the head's t, an inference unit with the
identity affine epilogue); behind LeakyReLU / Mish / a residual the same bar against the epilogue of the rounded operands'
convolution holds and the fp16 result must differ from the fp32 one.
The head unit needs Cout = A (5 + C) >= 32 (three anchors with two classes are 21 channels, which the engine runs on the
exact kernel): its cases use C = 6 (33 channels: one full tile column and one single column) and C = 20."""
import functools
import math
import os
import subprocess
import sys
from ctypes import byref, c_int, c_void_p

import pytest
import torch

from oracle import layers as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARG = -1          # YOLO_ERR_INVALID_ARG
BAR_ARITH = 2e-5          # of max|y|, against the float64 convolution of the rounded operands
BAR_ON = 1e-4             # of max|y|, against the float64 convolution of the unrounded operands
WIN, SK, PATCH = 0, 2, 5  # yolo_set_option keys

# (id, options, (N, H, W, Cin, Cout, k, stride, padding, bias)). Cin 16 = one channel block (the prologue runs on dummy
# stages), 48 = an odd block count (register-set parity), Cout 32 = the minimum, 80 / 160 = a partial tile column, pixel counts
# 63 and 480 are no multiples of a tile
FAMILIES = [
    # per-tap streaming kernel (window kernels off)
    ("stream-1x1-c16-o32", {WIN: 0, SK: 0}, (1, 7, 9, 16, 32, 1, 1, "same", False)),            # 128 x 32 tile, deeper ring
    ("stream-1x1-c48-o64", {WIN: 0, SK: 0}, (2, 12, 20, 48, 64, 1, 1, "same", False)),          # 128 x 64 tile, deeper ring
    ("stream-1x1-c48-o80", {WIN: 0, SK: 0}, (2, 12, 20, 48, 80, 1, 1, "same", True)),           # 128 x 128, eight waves
    ("stream-3x3-c48-o32", {WIN: 0, SK: 0}, (2, 12, 20, 48, 32, 3, 1, "same", False)),          # ONE MFMA per stage, four DMAs
    ("stream-3x3-c16-o80", {WIN: 0, SK: 0}, (1, 7, 9, 16, 80, 3, 1, "same", True)),             # 128 x 128, four waves
    ("stream-3x3s2-c16-o64", {WIN: 0, SK: 0}, (1, 7, 9, 16, 64, 3, 2, "darknet_s2", False)),
    ("stream-3x3s2-c48-o80", {WIN: 0, SK: 0}, (2, 12, 20, 48, 80, 3, 2, "darknet_s2", False)),
    ("stream-split-3x3s2-c48-o80", {WIN: 0, SK: 1}, (2, 12, 20, 48, 80, 3, 2, "darknet_s2", True)),   # split-K: 3 parts
    ("stream-split-1x1-c256-o128", {WIN: 0, SK: 1}, (1, 7, 9, 256, 128, 1, 1, "same", False)),       # split-K: 2 parts
    # window kernel, 128 x 128 and 256 x 128 tiles; stream-K forced onto five workgroups, stream-K by its own policy
    ("win2-c16-o160", {WIN: 2, SK: 0}, (1, 7, 9, 16, 160, 3, 1, "same", True)),
    ("win2-c48-o160", {WIN: 2, SK: 0}, (2, 12, 20, 48, 160, 3, 1, "same", False)),
    ("win4-c16-o160", {WIN: 4, SK: 0}, (1, 7, 9, 16, 160, 3, 1, "same", False)),
    ("win4-c48-o160", {WIN: 4, SK: 0}, (2, 12, 20, 48, 160, 3, 1, "same", True)),
    ("win2-split-c80-o128", {WIN: 2, SK: 1}, (2, 12, 20, 80, 128, 3, 1, "same", False)),        # parts of 2 and 3 blocks
    ("win2-streamk5-c48-o160", {WIN: 2, SK: 5}, (2, 12, 20, 48, 160, 3, 1, "same", False)),
    ("win4-streamk5-c48-o160", {WIN: 4, SK: 5}, (2, 12, 20, 48, 160, 3, 1, "same", False)),
    ("win2-streamk-c512-o128", {WIN: 2, SK: -1}, (1, 7, 9, 512, 128, 3, 1, "same", False)),
    # patch form of the window kernel: 256 x 64 tiles (Cout 64) and 128 x 128 tiles
    ("patch-c16-o64", {PATCH: 2}, (1, 7, 9, 16, 64, 3, 1, "same", False)),
    ("patch-c48-o160", {PATCH: 2}, (2, 12, 20, 48, 160, 3, 1, "same", True)),
]
_FAM = {f[0]: f for f in FAMILIES}
EPI_FAMILIES = ["stream-1x1-c48-o80", "stream-3x3-c48-o32", "stream-split-3x3s2-c48-o80", "win2-c48-o160",
                "win2-split-c80-o128", "patch-c16-o64"]

# inference units: (id, case). 1 x 5 x 6 with 64 -> 96 is conv_small's 32 x 32 tile (k = 1) and, for k = 3, the per-tap
# split-K pair whose reduce kernel writes the planes -- or conv_small under YOLO_CONV_SMALL=3 (the child-process test below)
UNITS = [
    ("small-1x1-c64-o96", (1, 5, 6, 64, 96, 1, 1, "same", False)),
    ("small-3x3-c64-o96", (1, 5, 6, 64, 96, 3, 1, "same", True)),
    ("small-1x1-c64-o128-tile22", (1, 52, 52, 64, 128, 1, 1, "same", False)),    # 340 tiles of 32 x 32 -> the 64 x 64 tile
    ("small-3x3-c32-o256-tile22", (1, 46, 46, 32, 256, 3, 1, "same", False)),    # 136 tiles of 64 x 64, 18 steps on 8 waves
    ("small-3x3s2-c48-o64", (2, 9, 11, 48, 64, 3, 2, "same", False)),
    ("unit-two-pass-1x1-c16-o128", (4, 72, 72, 16, 128, 1, 1, "same", False)),   # tiles fill the chip: conv + planes pass
]
# detection heads: (id, N, H, W, Cin, A, C, version)
HEADS = [
    ("head-v3-c6", 1, 5, 6, 64, 3, 6, 3),
    ("head-v4-c6", 1, 5, 6, 64, 3, 6, 4),
    ("head-v3-c20-tile22", 2, 52, 52, 64, 3, 20, 3),     # Cout 75 on the 64 x 64 tile
    ("head-v4-c6-streaming", 4, 48, 48, 16, 3, 6, 4),    # too many pixels for conv_small: convolution + activation kernels
]


def _scale_of(bound):
    """planes_scale_from_bound (csrc/planes.hpp): the power of two s with s * bound <= 2^15"""
    _, e = math.frexp(float(bound))
    return 2.0 ** (15 - e)


def _rounded(t32):
    """fp16(s t) / s as float64: what the h plane of t's planes holds"""
    s = _scale_of(t32.abs().max())
    return (t32 * s).half().double() / s


@functools.lru_cache(maxsize=None)
def _data(case, exact):
    """operands (fp32, CPU; the filter as [Cout][k][k][Cin]) and the float64 convolutions of the rounded / unrounded ones"""
    n, h, w, cin, cout, k, s, pad, bias = case
    g = torch.Generator().manual_seed(0)
    if exact:
        x = torch.randint(-8, 9, (n, h, w, cin), generator=g).float() / 64
        wk = torch.randint(-8, 9, (cout, k, k, cin), generator=g).float() / 64
        x[0, 0, 0, 0], wk[0, 0, 0, 0] = 0.125, -0.125   # (both bounds exactly 8 / 64)
    else:
        x = torch.randn(n, h, w, cin, generator=g).float()
        wk = (torch.randn(cout, k, k, cin, generator=g) / (k * k * cin) ** 0.5).float()
    b = (torch.randn(cout, generator=g) * 0.5).float() if bias else None
    out = {"x": x, "w": wk, "b": b}
    if not exact:
        hwio = lambda t: t.permute(1, 2, 3, 0).contiguous()
        bd = None if b is None else b.double()
        out["half"] = L.conv2d(_rounded(x), hwio(_rounded(wk)), bd, stride=s, padding=pad)
        out["full"] = L.conv2d(x.double(), hwio(wk.double()), bd, stride=s, padding=pad)
    return out


def _relerr(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


class _Options:
    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from tf2_yolo_amd import ops
        ops.ensure_conv_workspace()
        for k, v in self.opts.items():
            ops.set_option(k, v)

    def __exit__(self, *exc):
        from tf2_yolo_amd import ops
        ops.reset_options()


def _device_operands(case, exact):
    from tf2_yolo_amd import ops
    n, h, w, cin, cout, k, s, pad, bias = case
    dt = _data(case, exact)
    d = ops.conv_desc((n, h, w, cin), cout, k, k, s, pad)
    xd, wd = dt["x"].cuda(), dt["w"].cuda()
    bd = None if dt["b"] is None else dt["b"].cuda()
    return dt, d, xd, wd, bd, ops.split_planes(xd, n * h * w, cin), ops.split_planes(wd, cout, k * k * cin)


def _plain(d, xp, wp, bd, precision):
    from tf2_yolo_amd import ops
    amax = torch.zeros(d.Cout, device="cuda", dtype=torch.int32)
    y = ops.conv2d_fwd_planes(d, xp, wp, bd, absmax=amax, precision=precision)
    torch.cuda.synchronize()
    return y, amax


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(0 if t is None else t.data_ptr())


def test_h_plane_is_the_fp16_rounding_of_the_scaled_operand():
    """the reference of this file: plane h of yolo_split_planes == fp16(s x) (round to nearest even), s from max|x|"""
    from tf2_yolo_amd import ops
    rows, c = 63, 48
    x = _data((1, 7, 9, 48, 32, 1, 1, "same", False), False)["x"].reshape(rows, c)
    pl = ops.split_planes(x.cuda(), rows, c).cpu()
    nblk = (rows + 15) // 16
    body = (nblk + 1) * (c // 16) * 1024
    hdr = pl[body:body + 12].clone().view(torch.float32)
    u = pl[:body].clone().view(torch.float16).reshape(nblk + 1, c // 16, 2, 2, 16, 8)      # [blk][kb][plane][half][row][8]
    hpl = u.permute(2, 0, 4, 1, 3, 5).reshape(2, (nblk + 1) * 16, c)[0, :rows]
    assert float(hdr[1]) == _scale_of(x.abs().max())
    assert torch.equal(hpl.double() / float(hdr[1]), _rounded(x))


@pytest.mark.parametrize("fam", [f[0] for f in FAMILIES])
def test_exact_operands_give_the_fp32_mode_result_bit_for_bit(fam):
    _, opts, case = _FAM[fam]
    dt, d, xd, wd, bd, xp, wp = _device_operands(case, True)
    with _Options(opts):
        y32, a32 = _plain(d, xp, wp, bd, "fp32")
        y16, a16 = _plain(d, xp, wp, bd, "fp16")
    assert float(y32.abs().max()) > 0
    assert torch.equal(y16, y32) and torch.equal(a16, a32)
    assert torch.equal(a16.view(torch.float32), y16.reshape(-1, d.Cout).abs().max(0).values)


@pytest.mark.parametrize("fam", [f[0] for f in FAMILIES])
def test_one_pass_is_the_convolution_of_the_rounded_operands(fam):
    from tf2_yolo_amd import _lib
    _, opts, case = _FAM[fam]
    dt, d, xd, wd, bd, xp, wp = _device_operands(case, False)
    with _Options(opts):
        y32, a32 = _plain(d, xp, wp, bd, "fp32")
        y16, a16 = _plain(d, xp, wp, bd, "fp16")
        # the entry point without the suffix
        y0, a0 = torch.empty_like(y32), torch.zeros_like(a32)
        rc = _lib.load().yolo_conv2d_fwd_planes(byref(d), _ptr(xp), _ptr(wp), _ptr(bd), _ptr(y0), None, _ptr(a0), _stream())
        torch.cuda.synchronize()
    assert rc == 0 and torch.equal(y0, y32) and torch.equal(a0, a32)                 # default untouched
    e_half, e_full = _relerr(y16.double().cpu(), dt["half"]), _relerr(y16.double().cpu(), dt["full"])
    e32 = _relerr(y32.double().cpu(), dt["full"])
    print(f"{fam}: fp16 vs rounded-operand conv {e_half:.3g}, vs unrounded {e_full:.3g}; fp32 vs unrounded {e32:.3g}")
    assert e_half < BAR_ARITH                                                        # the right arithmetic
    assert e_full > BAR_ON                                                           # the feature is on
    assert e32 < BAR_ARITH
    assert torch.equal(a16.view(torch.float32), y16.reshape(-1, d.Cout).abs().max(0).values)


def _epilogue_ref(conv, scale, shift, act, res):
    z = conv * scale.double().cpu() + shift.double().cpu()
    z = L.leaky(z) if act == "leaky" else L.mish(z) if act == "mish" else z
    return z + (res.double().cpu() if res is not None else 0.0)


def _affine(cout, with_res, shape, exact):
    g = torch.Generator().manual_seed(3)
    scale = ((torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0)).float().cuda()
    shift = (torch.randn(cout, generator=g) * 0.3).float().cuda()
    res = (torch.randn(*shape, generator=g) * (0.125 if exact else 1.0)).float().cuda() if with_res else None
    return scale, shift, res


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", ["leaky", "mish"])
@pytest.mark.parametrize("fam", EPI_FAMILIES)
def test_fused_epilogue_forms(fam, act, with_res):
    """yolo_conv2d_fwd_planes_epi_ex: folded BatchNorm + LeakyReLU / Mish (+ residual) behind one pass, the reduce kernel of
    the split-K forms included"""
    from tf2_yolo_amd import _lib, ops
    _, opts, case = _FAM[fam]
    epi = ops.EPI_AFFINE_LEAKY if act == "leaky" else ops.EPI_AFFINE_MISH
    for exact in (True, False):
        dt, d, xd, wd, bd, xp, wp = _device_operands(case, exact)
        scale, shift, res = _affine(d.Cout, with_res, (d.N, d.Ho, d.Wo, d.Cout), exact)

        def run(precision):
            amax = torch.zeros(d.Cout, device="cuda", dtype=torch.int32)
            y = ops.conv2d_fwd_planes_epi(d, xp, wp, bd, epi, scale, shift, residual=res, absmax=amax, precision=precision)
            torch.cuda.synchronize()
            return y, amax
        with _Options(opts):
            y32, a32 = run("fp32")
            y16, a16 = run("fp16")
            y0, a0 = torch.empty_like(y32), torch.zeros_like(a32)
            rc = _lib.load().yolo_conv2d_fwd_planes_epi(byref(d), _ptr(xp), _ptr(wp), _ptr(bd), int(epi), _ptr(scale),
                                                        _ptr(shift), _ptr(res), _ptr(y0), _ptr(a0), _stream())
            torch.cuda.synchronize()
        assert rc == 0 and torch.equal(y0, y32) and torch.equal(a0, a32)
        if exact:
            assert torch.equal(y16, y32) and torch.equal(a16, a32)
        else:
            e_half = _relerr(y16.double().cpu(), _epilogue_ref(dt["half"], scale, shift, act, res))
            e32 = _relerr(y32.double().cpu(), _epilogue_ref(dt["full"], scale, shift, act, res))
            print(f"{fam} {act} res={with_res}: fp16 vs rounded-operand unit {e_half:.3g}; fp32 vs unrounded {e32:.3g}")
            assert e_half < BAR_ARITH and e32 < BAR_ARITH
            assert not torch.equal(y16, y32)


def _unit(d, xp, wp, bd, epi, scale, shift, res, in_bound, res_bound, pred, precision):
    from tf2_yolo_amd import ops
    rows = d.N * d.Ho * d.Wo
    y = torch.full((d.N, d.Ho, d.Wo, d.Cout), float("nan"), device="cuda")
    amax = torch.zeros(d.Cout, device="cuda", dtype=torch.int32)
    pl = torch.zeros(ops.planes_bytes(rows, d.Cout), device="cuda", dtype=torch.uint8)
    words = torch.full((ops.INFER_BOUND_WORDS,), -1, device="cuda", dtype=torch.int32)
    ob = torch.zeros(1, device="cuda")
    nw = ops.conv2d_fwd_infer_unit(d, xp, wp, bd, epi, scale, shift, res, y, amax, pred, in_bound, res_bound, pl, words, ob,
                                   precision=precision)
    torch.cuda.synchronize()
    return {"y": y, "amax": amax, "planes": pl, "words": words, "bound": ob, "nw": nw}


@pytest.mark.parametrize("act,with_res", [("linear", False), ("leaky", True), ("mish", False), ("mish", True)])
@pytest.mark.parametrize("unit", [u[0] for u in UNITS])
def test_inference_unit(unit, act, with_res):
    """yolo_conv2d_fwd_infer_unit_ex (conv_small.hip, the split-K pair, the two-pass form): y, absmax, the planes going out and
    the bound words. "linear" is the identity affine epilogue: y is the convolution itself."""
    from tf2_yolo_amd import _lib, ops
    case = dict(UNITS)[unit]
    epi = {"linear": ops.EPI_AFFINE, "leaky": ops.EPI_AFFINE_LEAKY, "mish": ops.EPI_AFFINE_MISH}[act]
    ops.ensure_conv_workspace()
    for exact in (True, False):
        dt, d, xd, wd, bd, xp, wp = _device_operands(case, exact)
        scale, shift, res = _affine(d.Cout, with_res, (d.N, d.Ho, d.Wo, d.Cout), exact)
        if act == "linear":
            scale, shift = torch.ones_like(scale), torch.zeros_like(shift)
        pred = torch.zeros(2, device="cuda")
        ops.conv_pred_bound(wd, d.Cout, d.kh * d.kw * d.Cin, scale, shift, bd, pred)
        in_bound = xd.abs().max().reshape(1)
        res_bound = res.abs().max().reshape(1) if with_res else None
        r32 = _unit(d, xp, wp, bd, epi, scale, shift, res, in_bound, res_bound, pred, "fp32")
        r16 = _unit(d, xp, wp, bd, epi, scale, shift, res, in_bound, res_bound, pred, "fp16")
        # the entry point without the suffix
        r0 = {k: torch.full_like(v, -1) if k == "words" else torch.zeros_like(v) for k, v in r32.items() if k != "nw"}
        n0 = c_int(0)
        rc = _lib.load().yolo_conv2d_fwd_infer_unit(
            byref(d), _ptr(xp), _ptr(wp), _ptr(bd), int(epi), _ptr(scale), _ptr(shift), _ptr(res), _ptr(r0["y"]), _ptr(r0["amax"]),
            _ptr(pred), _ptr(in_bound), 1, _ptr(res_bound), 1 if with_res else 0, _ptr(r0["planes"]), _ptr(r0["words"]),
            _ptr(r0["bound"]), byref(n0), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and n0.value == r32["nw"]
        for k, v in r0.items():
            assert torch.equal(v, r32[k]), (k, "default untouched")
        assert r16["nw"] == r32["nw"]                         # the same kernels in both modes
        if exact:
            for k, v in r0.items():
                assert torch.equal(r16[k], r32[k]), k
            continue
        y16 = r16["y"].double().cpu()
        e_half = _relerr(y16, _epilogue_ref(dt["half"], scale, shift, act, res))
        e_full = _relerr(y16, _epilogue_ref(dt["full"], scale, shift, act, res))
        e32 = _relerr(r32["y"].double().cpu(), _epilogue_ref(dt["full"], scale, shift, act, res))
        print(f"{unit} {act} res={with_res}: fp16 vs rounded {e_half:.3g}, vs unrounded {e_full:.3g}; fp32 vs unrounded {e32:.3g}")
        assert e_half < BAR_ARITH and e32 < BAR_ARITH
        assert not torch.equal(r16["y"], r32["y"])
        if act == "linear":
            assert e_full > BAR_ON
        # the planes going out hold the fp16-mode y (both planes are written), under the same a-priori scale
        from planes_util import planes_to_dense
        rows = d.N * d.Ho * d.Wo
        vals, bound, sc, tail = planes_to_dense(r16["planes"].cpu(), rows, d.Cout)
        yd = y16.reshape(rows, d.Cout)
        assert tail and bound >= float(yd.abs().max())
        assert ((vals - yd).abs() <= torch.maximum(2.0 ** -22 * yd.abs(), torch.tensor(2.0 ** -25 / sc, dtype=torch.float64))).all()
        if r16["nw"]:
            assert float(r16["words"][:r16["nw"]].view(torch.float32).max()) == float(r16["y"].abs().max())


@pytest.mark.parametrize("head", [h[0] for h in HEADS])
def test_head_unit(head):
    """yolo_conv2d_fwd_head_unit_ex: t = the 1x1 convolution + bias, y = the head's activation of the t this call wrote"""
    from tf2_yolo_amd import _lib, ops
    _, n, h, w, cin, A, C, version = {x[0]: x for x in HEADS}[head]
    cout = A * (5 + C)
    case = (n, h, w, cin, cout, 1, 1, "same", True)
    ops.ensure_conv_workspace()
    anchors = (torch.rand(A, 2, generator=torch.Generator().manual_seed(5)) + 0.1).float().cuda()
    for exact in (True, False):
        dt, d, xd, wd, bd, xp, wp = _device_operands(case, exact)

        def run(precision):
            t, y = torch.full((n, h, w, cout), float("nan"), device="cuda"), torch.full((n, h, w, cout), float("nan"), device="cuda")
            ops.conv2d_fwd_head_unit(d, xp, wp, bd, A, C, version, anchors, t, y, precision=precision)
            torch.cuda.synchronize()
            return t, y
        t32, y32 = run("fp32")
        t16, y16 = run("fp16")
        t0, y0 = torch.empty_like(t32), torch.empty_like(t32)
        rc = _lib.load().yolo_conv2d_fwd_head_unit(byref(d), _ptr(xp), _ptr(wp), _ptr(bd), A, C, version, _ptr(anchors), _ptr(t0),
                                                   _ptr(y0), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(t0, t32) and torch.equal(y0, y32)
        assert torch.equal(y16, ops.head_act_fwd(t16, A, C, version, anchors))
        if exact:
            assert torch.equal(t16, t32) and torch.equal(y16, y32)
            continue
        e_half, e_full = _relerr(t16.double().cpu(), dt["half"]), _relerr(t16.double().cpu(), dt["full"])
        e32 = _relerr(t32.double().cpu(), dt["full"])
        print(f"{head}: fp16 t vs rounded-operand conv {e_half:.3g}, vs unrounded {e_full:.3g}; fp32 vs unrounded {e32:.3g}")
        assert e_half < BAR_ARITH and e_full > BAR_ON and e32 < BAR_ARITH


def test_argument_handling():
    """BatchNorm statistics (the training forward) with YOLO_PREC_F16, and a precision that is neither enumerator, return
    YOLO_ERR_INVALID_ARG from every _ex entry point and write nothing; the ops wrappers raise"""
    from tf2_yolo_amd import _lib, ops
    lib = _lib.load()
    case = (1, 7, 9, 16, 32, 1, 1, "same", False)
    dt, d, xd, wd, bd, xp, wp = _device_operands(case, True)
    y = torch.full((1, 7, 9, 32), 7.0, device="cuda")
    stats = torch.zeros(ops.BN_STAT_SLOTS * 2 * 32, device="cuda", dtype=torch.float64)
    amax = torch.zeros(32, device="cuda", dtype=torch.int32)
    assert lib.yolo_conv2d_fwd_planes_ex(byref(d), _ptr(xp), _ptr(wp), None, _ptr(y), _ptr(stats), _ptr(amax), _lib.PREC_F16,
                                         _stream()) == INVALID_ARG
    assert b"statistics" in lib.yolo_last_error()
    for bad in (2, -1, 16):
        assert lib.yolo_conv2d_fwd_planes_ex(byref(d), _ptr(xp), _ptr(wp), None, _ptr(y), None, _ptr(amax), bad,
                                             _stream()) == INVALID_ARG
        assert b"precision" in lib.yolo_last_error()
        sc, sh = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
        assert lib.yolo_conv2d_fwd_planes_epi_ex(byref(d), _ptr(xp), _ptr(wp), None, ops.EPI_AFFINE, _ptr(sc), _ptr(sh), None,
                                                 _ptr(y), _ptr(amax), bad, _stream()) == INVALID_ARG
        pred, words, ob, nw = torch.zeros(2, device="cuda"), torch.zeros(4096, device="cuda", dtype=torch.int32), \
            torch.zeros(1, device="cuda"), c_int(0)
        pl = torch.zeros(ops.planes_bytes(63, 32), device="cuda", dtype=torch.uint8)
        assert lib.yolo_conv2d_fwd_infer_unit_ex(byref(d), _ptr(xp), _ptr(wp), None, ops.EPI_AFFINE, _ptr(sc), _ptr(sh), None,
                                                 _ptr(y), _ptr(amax), _ptr(pred), _ptr(ob), 1, None, 0, _ptr(pl), _ptr(words),
                                                 _ptr(ob), byref(nw), bad, _stream()) == INVALID_ARG
        anchors = torch.ones(4, 2, device="cuda")
        assert lib.yolo_conv2d_fwd_head_unit_ex(byref(d), _ptr(xp), _ptr(wp), None, 4, 3, 3, _ptr(anchors), _ptr(y), _ptr(y),
                                                bad, _stream()) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not bool(stats.any()) and not bool(amax.any())
    with pytest.raises(_lib.YoloHipError):
        ops.conv2d_fwd_planes(d, xp, wp, None, stats=stats, precision="fp16")
    with pytest.raises(ValueError):
        ops.conv2d_fwd_planes(d, xp, wp, None, precision="int8")
    # the training form itself is untouched: statistics with fp32
    ops.conv2d_fwd_planes(d, xp, wp, None, out=y, stats=stats, precision="fp32")
    torch.cuda.synchronize()
    assert bool(stats.any())


@pytest.mark.parametrize("env", [{"YOLO_CONV_SMALL": "3"}, {"YOLO_CONV_SMALL": "3", "YOLO_CONV_SMALL_TILE": "21"}],
                         ids=lambda e: " ".join(f"{k}={v}" for k, v in e.items()))
def test_conv_small_forms_the_library_policy_reads_once(env):
    """conv_small's 3x3 forms on the 32 x 32 tile and every form on the 64 x 32 tile are chosen by switches the library reads
    once per process: the inference-unit cases of this file run again in a child process under them"""
    child_env = dict(os.environ)
    child_env.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                        "test_inference_unit and small and not tile22"], cwd=ROOT, env=child_env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout.strip().splitlines()[-1])
