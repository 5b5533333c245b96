"""The chain logits -> head -> loss -> gradient at SATURATED predictions (tests/saturation_cases.py): confidences and class
probabilities at, next to and beyond the float32 clip bounds of the losses, widths at the ends of the finite range, head
logits where sigmoid / softmax / exp saturate. References: oracle/losses.py (float64, the reference's float32 clip bounds),
oracle/metrics.py, and the float64 NumPy head of saturation_cases. That the cases hold every edge value in every kind of
cell, that no decision hangs on the precision of an IoU and that the reference is finite on them is asserted GPU-free by
tests/test_saturation_cases_cpu.py.

Bars. Loss: the suite's 1e-4 max(|ref|, 1) on the total and every part, 1e-4 of the largest reference entry of a channel
kind (xy, wh, conf, cls) on the gradient. Head: 1e-6 of the largest reference entry of the kind -- an expf of at most one
unit in the last place (6e-8) and at most eight float32 roundings (8 x 2^-24 = 4.8e-7) in any of its expressions."""
import functools

import numpy as np
import pytest
import torch

import saturation_cases as SC
from oracle import metrics as OM

pytestmark = pytest.mark.gpu
TOL = 1e-4
HEAD_TOL = 1e-6
KIND_NAMES = ("xy", "wh", "conf", "cls")
PARTS_V3 = ("xy", "wh", "conf_obj", "conf_noobj", "prob", "reg")


def _cfg(case):
    from tf2_yolo_amd import ops
    args, kw = SC.cfg_args(case)
    return ops.make_loss_cfg(*args, **kw)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = {c.name: c for c in SC.CLIP_CASES + SC.WIDTH_CASES}[name]
    return SC.clip_inputs(case) if case in SC.CLIP_CASES else SC.width_inputs(case)


def _oracle(case, yt, yp):
    """float64 oracle on float32 inputs: (loss, parts or None, gradient as float64 array)"""
    p = torch.tensor(yp, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(yt, dtype=torch.float64)
    parts = None
    if case.version == 3:
        loss, parts = SC.oracle_fn(case, parts=True)(t, p)
        parts = {k: v.item() for k, v in parts.items()}
    else:
        loss = SC.oracle_fn(case)(t, p)
    loss.backward()
    return loss.item(), parts, p.grad.numpy()


@functools.lru_cache(maxsize=None)
def _oracle_of(name):
    case = {c.name: c for c in SC.CLIP_CASES + SC.WIDTH_CASES}[name]
    return _oracle(case, *_inputs(name))


def _check_loss(case, yt, yp, ref, tag, clipped_outside=None):
    """ops.loss_fwd_bwd twice on (yt, yp) against ref = (loss, parts, gradient); returns the device's gradient (float32)"""
    from tf2_yolo_amd import ops
    ref_loss, ref_parts, ref_grad = ref
    ytd, ypd = torch.tensor(yt).cuda(), torch.tensor(yp).cuda()
    cfg = _cfg(case)
    runs = []
    for _ in range(2):
        out, dp = ops.loss_fwd_bwd(cfg, ytd, ypd)
        torch.cuda.synchronize()
        runs.append((out.cpu().numpy().copy(), dp.cpu().numpy().copy()))
    (out, dp), (out2, dp2) = runs
    # two runs: the gradient bit for bit, the sums up to the order of the per-workgroup fp64 atomics
    assert np.array_equal(dp.view(np.uint32), dp2.view(np.uint32))
    assert np.allclose(out[:7], out2[:7], rtol=1e-12, atol=0)
    assert np.isfinite(out[:7]).all() and np.isfinite(dp).all()
    err = abs(out[0] - ref_loss) / max(abs(ref_loss), 1.0)
    line = f"SATURATION_LOSS {tag}: total {out[0]:.6f} (oracle {ref_loss:.6f}) error {err:.2e}"
    assert err <= TOL, (out[0], ref_loss)
    if ref_parts is not None:
        for i, k in enumerate(PARTS_V3):
            assert abs(out[1 + i] - ref_parts[k]) <= TOL * max(abs(ref_parts[k]), 1.0), (k, out[1 + i], ref_parts[k])
    ck = SC.channel_kinds(case)
    PD = len(ck)
    g, r = dp.astype(np.float64).reshape(-1, PD), ref_grad.reshape(-1, PD)
    for k in KIND_NAMES:
        scale = np.abs(r[:, ck == k]).max()
        e = np.abs(g[:, ck == k] - r[:, ck == k]).max()
        line += f", d{k} {e / max(scale, 1e-300):.2e} of {scale:.3g}"
        assert scale > 0 and e <= TOL * scale, (k, e, scale)
    print(line)
    if clipped_outside is not None:
        assert clipped_outside.any() and np.all(dp.reshape(-1)[clipped_outside] == 0.0)
    return dp


def _clipped_outside(case, yp):
    """flat mask over y_pred: elements the loss clips (class channels; the confidence of a focal / v4 loss) whose value
    lies outside [lo, hi]"""
    ck = SC.channel_kinds(case)
    clipped = (ck == "cls") | ((ck == "conf") & SC.CONF_IS_CLIPPED(case))
    v = yp.reshape(-1, len(ck))
    return (clipped[None, :] & ((v < SC.LO) | (v > SC.HI))).reshape(-1)


@pytest.mark.parametrize("loader", ["default", "chunk-ahead"])
@pytest.mark.parametrize("case", SC.CLIP_CASES, ids=lambda c: c.name)
def test_loss_at_the_clip_bounds(case, loader):
    """every confidence and class probability is one of 0, the smallest subnormal, lo and hi and their neighbours, 0.5, 1:
    total, parts and gradient against the oracle with the reference's float32 bounds; the gradient is exactly 0 outside
    [lo, hi]; with the launcher's loader and with the chunk-ahead loader (ops.set_option(8, 8))"""
    from tf2_yolo_amd import ops
    yt, yp = _inputs(case.name)
    try:
        if loader == "chunk-ahead":
            ops.set_option(8, 8)
        _check_loss(case, yt, yp, _oracle_of(case.name), f"{case.name} {loader}", _clipped_outside(case, yp))
    finally:
        ops.reset_options()


@pytest.mark.parametrize("loader", ["default", "chunk-ahead"])
@pytest.mark.parametrize("case", SC.WIDTH_CASES, ids=lambda c: c.name)
def test_loss_at_the_ends_of_the_width_range(case, loader):
    """w, h = exp(t) anchor for t in -80 .. 9 (v1.5: p around 1e-7, 0 and 1) and one true width below 1e-7 anchor"""
    from tf2_yolo_amd import ops
    yt, yp = _inputs(case.name)
    try:
        if loader == "chunk-ahead":
            ops.set_option(8, 8)
        _check_loss(case, yt, yp, _oracle_of(case.name), f"{case.name} {loader}")
    finally:
        ops.reset_options()


@pytest.mark.parametrize("case", SC.CLIP_CASES, ids=lambda c: c.name)
def test_metrics_at_the_clip_bounds(case):
    from tf2_yolo_amd import ops
    yt, yp = _inputs(case.name)
    g, A, C = case.g, case.A, case.C
    out = ops.metrics(_cfg(case), torch.tensor(yt).cuda(), torch.tensor(yp).cuda(), recall_thresh=0.5).cpu().numpy()
    t, p = torch.tensor(yt, dtype=torch.float64), torch.tensor(yp, dtype=torch.float64)
    cells = case.N * g[0] * g[1]
    if case.version == 1:
        ref = [OM.obj_acc_v1(t, p, g, A, C).mean().item(), OM.mean_iou_v1(t, p, g, A, C).item(),
               OM.class_acc_v1(t, p, g, C).item(), OM.recall_v1(t, p, g, A, C, 0.5).item()]
        got = [out[0] / cells, out[1] / (out[2] + 1e-7), out[3] / (out[2] + 1e-7), out[4] / (out[2] + 1e-7)]
    else:
        ref = [OM.obj_acc(t, p, g, A, C).mean().item(), OM.mean_iou(t, p, g, A, C).item(),
               OM.class_acc(t, p, g, A, C).item(), OM.recall(t, p, g, A, C, 0.5).item()]
        got = [out[0] / cells, out[1] / (out[2] + 1e-7), out[3] / (out[2] * A + 1e-7), out[4] / (out[2] + 1e-7)]
    assert out[5] == cells and out[2] == float((t[..., 4] > 0).sum())
    for a, b in zip(got, ref):
        assert abs(a - b) < 1e-5, (got, ref)


# ---- the head ------------------------------------------------------------------------------------------------------
def _anchors32(version, A):
    """float32 anchors of a head (what the device holds) and the same numbers as float64 for the reference"""
    if version == 1:
        return None, None
    a = np.array((SC.ANCH5 if A == 5 else (SC.PC.ANCH9[:A])), dtype=np.float32)
    return torch.tensor(a.reshape(-1)).cuda(), a.astype(np.float64)


def _by_kind(arr, version, A, C):
    cols = SC.head_columns(version, A, C)
    a = np.asarray(arr, dtype=np.float64).reshape(-1, sum(len(c) for c in cols.values()))
    return {k: a[:, cols[k]] for k in KIND_NAMES}


def _compare_kinds(got, ref, tol, tag):
    line = tag
    for k in KIND_NAMES:
        scale = np.abs(ref[k]).max()
        e = np.abs(got[k] - ref[k]).max()
        line += f" {k} {e / max(scale, 1e-300):.2e}"
        assert e <= tol * scale, (tag, k, e, scale)
    print(line)


def _check_head_fwd(t, y, version, A, C, anc64, tag):
    """y = head(t) per channel kind against the float64 head, and its exact properties"""
    ref = SC.ref_head(t, version, A, C, anc64)
    got = _by_kind(y, version, A, C)
    assert np.isfinite(y).all()
    _compare_kinds(got, ref, HEAD_TOL, f"SATURATION_HEAD_FWD {tag}:")
    tk = _by_kind(t, version, A, C)
    sig = ["xy", "conf"] + (["wh"] if version == 1 else []) + ([] if SC.is_softmax(version) else ["cls"])
    tv = np.concatenate([tk[k].reshape(-1) for k in sig])
    yv = np.concatenate([got[k].reshape(-1) for k in sig])
    assert yv.min() >= 0.0 and yv.max() <= 1.0
    order = np.argsort(tv, kind="stable")
    assert np.all(np.diff(yv[order]) >= 0)                       # monotone in the logit (equal logits: equal outputs)
    assert np.all(yv[tv >= 18] == 1.0) and np.all(yv[tv <= -104] == 0.0)
    assert (tv >= 18).any() and (tv <= -104).any()
    if version != 1:
        assert got["wh"].min() > 0
    if SC.is_softmax(version):
        P = got["cls"].shape[0]
        rows, trows = got["cls"].reshape(P, -1, C), tk["cls"].reshape(P, -1, C)
        assert rows.min() >= 0.0 and rows.max() <= 1.0
        assert np.abs(rows.sum(-1) - 1).max() <= 1e-6
        o = np.argsort(trows, axis=-1, kind="stable")
        assert np.all(np.diff(np.take_along_axis(rows, o, -1), axis=-1) >= 0)
        top = trows.max(-1, keepdims=True)
        if C > 1:
            far = trows <= top - 104                                 # expf(-104) is 0
            assert far.any() and np.all(rows[far] == 0.0)
            won = np.sort(trows, -1)[..., -2] <= top[..., 0] - 104   # every other logit that far below: exactly 1
            assert won.any() and np.all(rows.max(-1)[won] == 1.0)
        equal = (trows == top).all(-1)
        assert equal.any() and np.all(np.abs(rows[equal] - 1.0 / C) <= 2.0 ** -24)


def _softmax_flat(y, C):
    """where y (dy - sum(dy y)) is exactly 0 whatever dy is: y = 0, and y = 1 with every other entry of its row 0 (a 1.0f
    beside a 3e-8 is a rounded 1: sum(dy y) is not dy there)"""
    rows = y.reshape(y.shape[0], -1, C)
    one_hot = ((rows == 0.0) | (rows == 1.0)).all(-1, keepdims=True)
    return ((rows == 0.0) | ((rows == 1.0) & one_hot)).reshape(y.shape)


@pytest.mark.parametrize("version,A,C", [(3, 3, 3), (4, 3, 1), (3, 3, 80), (2, 5, 3), (1, 2, 3), (1, 2, 1)])
def test_head_on_the_logit_table(version, A, C):
    """yolo_head_act_fwd / _bwd on logits from 0 to +-200 (expf overflows at 88.7, sigmoid is 1.0f above 16.6), widths
    exp(-80) .. exp(9), and softmax rows with one logit 200 above the rest, all equal, all -200"""
    from tf2_yolo_amd import ops
    t = SC.head_logits(version, A, C)
    anc, anc64 = _anchors32(version, A)
    td = torch.tensor(t).cuda()
    yd = ops.head_act_fwd(td, A, C, version, anc)
    y = yd.cpu().numpy()
    _check_head_fwd(t, y, version, A, C, anc64, f"v{version} A={A} C={C}")
    rng = np.random.default_rng(version * 100 + C)
    dy = rng.standard_normal(t.shape).astype(np.float32)
    dt = ops.head_act_bwd(yd, torch.tensor(dy).cuda(), A, C, version, anc).cpu().numpy()
    assert np.isfinite(dt).all()
    _compare_kinds(_by_kind(dt, version, A, C), SC.ref_head_bwd(y, dy, version, A, C), HEAD_TOL,
                   f"SATURATION_HEAD_BWD v{version} A={A} C={C}:")
    yk, dk = _by_kind(y, version, A, C), _by_kind(dt, version, A, C)
    for k in ("xy", "conf", "cls") + (("wh",) if version == 1 else ()):
        flat = _softmax_flat(yk[k], C) if k == "cls" and SC.is_softmax(version) else (yk[k] == 0.0) | (yk[k] == 1.0)
        assert (flat & (yk[k] == 1.0)).any() and np.all(dk[k][flat] == 0.0)
        assert (flat & (yk[k] == 0.0)).any() or (k == "cls" and C == 1 and SC.is_softmax(version))   # (softmax of one class is 1)


@pytest.mark.parametrize("case", SC.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_logits_head_loss_gradient(case):
    """stage by stage, each stage's reference on the device's own previous output: head(t) against the float64 head; the
    loss of the device's float32 y against the oracle on that y; the head's backward of the device's dL/dy against the
    float64 backward. The chain holds predictions clipped at both ends, and their logits get a gradient of exactly 0."""
    from tf2_yolo_amd import ops
    v, A, C = case.version, case.A, case.C
    yt, t = SC.chain_inputs(case)
    PD = t.shape[-1]
    anc, anc64 = _anchors32(v, A)
    if anc64 is not None:
        assert np.array_equal(anc64, np.array(case.anchors, dtype=np.float32).astype(np.float64))
    # stage 1
    yd = ops.head_act_fwd(torch.tensor(t).cuda(), A, C, v, anc)
    y = yd.cpu().numpy()
    ref = SC.ref_head(t.reshape(-1, PD), v, A, C, anc64)
    assert np.isfinite(y).all()
    _compare_kinds(_by_kind(y, v, A, C), ref, HEAD_TOL, f"SATURATION_CHAIN {case.name} head:")
    # stage 2
    outside = _clipped_outside(case, y)
    low, high = outside & (y.reshape(-1) < SC.LO), outside & (y.reshape(-1) > SC.HI)
    assert low.any() and high.any()
    dp = _check_loss(case, yt, y, _oracle(case, yt, y), f"{case.name} loss", outside)
    # stage 3
    dt = ops.head_act_bwd(yd, torch.tensor(dp).cuda(), A, C, v, anc).cpu().numpy()
    assert np.isfinite(dt).all()
    _compare_kinds(_by_kind(dt, v, A, C), SC.ref_head_bwd(y.reshape(-1, PD), dp.reshape(-1, PD), v, A, C), HEAD_TOL,
                   f"SATURATION_CHAIN {case.name} head backward:")
    ck = SC.channel_kinds(case)
    exact = outside.copy()
    if SC.is_softmax(v):   # dt_c = y_c (g_c - sum g y): exactly 0 with g_c = 0 only where y_c is 0 (or 1, the others 0)
        y2 = y.reshape(-1, PD)
        flat = np.ones(y2.shape, dtype=bool)
        flat[:, ck == "cls"] = _softmax_flat(y2[:, ck == "cls"], C)
        exact &= flat.reshape(-1)
    assert (exact & low).any() and (exact & high).any()
    assert np.all(dt.reshape(-1)[exact] == 0.0)


# ---- the fused head ------------------------------------------------------------------------------------------------------
# (version, A, C, images, grid, tile): tile 11 = 32 x 32, 22 = 64 x 64 (csrc/conv_small.hip: small_head_tile), None = v2, whose
# softmax keeps convolution + yolo_head_act_fwd behind the same entry. The unit takes Cout >= 32: four anchors at C = 3.
FUSED = [(3, 4, 3, 1, 13, 11), (4, 4, 3, 2, 76, 22), (4, 3, 80, 1, 13, 11), (3, 3, 80, 1, 52, 22),
         (2, 5, 3, 1, 13, None), (2, 5, 80, 1, 13, None)]


@pytest.mark.parametrize("version,A,C,n,hw,tile", FUSED)
def test_fused_head_on_the_logit_table(version, A, C, n, hw, tile):
    """yolo_conv2d_fwd_head_unit with all-zero filters and the logit table as its bias: t is the bias, y is bit for bit
    yolo_head_act_fwd of that t (conv_small.hip restates the head's expressions) and meets the float64 head"""
    import os
    from test_gpu_conv import _conv_small_head_tile
    from tf2_yolo_amd import ops
    ops.ensure_conv_workspace()
    cout, cin = A * (5 + C), 16
    if tile is not None:
        assert _conv_small_head_tile(n * hw * hw, cout) == (0 if os.environ.get("YOLO_CONV_SMALL") == "0" else tile)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, hw, hw, cin, generator=g).float().cuda()
    wk = torch.zeros(cout, cin).cuda()
    bias = SC.head_bias(A, C)
    a = np.array((SC.ANCH5 if A == 5 else [[0.9, 0.8], [0.4, 0.5], [0.3, 0.2], [0.1, 0.3]][:A]), dtype=np.float32)
    anc = torch.tensor(a.reshape(-1)).cuda()
    d = ops.conv_desc((n, hw, hw, cin), cout, 1, 1, 1, "same")
    xp = ops.split_planes(x, n * hw * hw, cin)
    wp = ops.split_planes(wk, cout, cin)
    t = torch.full((n, hw, hw, cout), float("nan"), device="cuda")
    y = torch.full((n, hw, hw, cout), float("nan"), device="cuda")
    ops.conv2d_fwd_head_unit(d, xp, wp, torch.tensor(bias).cuda(), A, C, version, anc, t, y)
    torch.cuda.synchronize()
    tc = t.cpu().numpy().reshape(-1, cout)
    assert np.array_equal(tc, np.broadcast_to(bias, tc.shape))
    y2 = ops.head_act_fwd(t, A, C, version, anc)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), y2.cpu().numpy().view(np.uint32))
    yc = y.cpu().numpy().reshape(-1, cout)
    assert np.isfinite(yc).all() and np.array_equal(yc, np.broadcast_to(yc[0], yc.shape))
    ref = SC.ref_head(bias.reshape(1, -1), version, A, C, a.astype(np.float64))
    _compare_kinds(_by_kind(yc[:1], version, A, C), ref, HEAD_TOL, f"SATURATION_FUSED v{version} A={A} C={C} {hw}x{hw}:")
