"""GPU-free guards of the saturation tests (tests/saturation_cases.py):

  * every clip case holds every edge value in every kind of cell and channel the loss distinguishes, and no IoU of any case
    comes near a threshold: float32 and float64 take the same branches, so a disagreement of the device with the float64
    oracle is a fault of the kernel;
  * the oracle evaluated in float32 is finite on every case -- the cases stay inside the range where the reference itself
    is finite (widths exp(-80) .. exp(9) times the anchor);
  * the clip cases tell the two upper clip bounds apart: with CLIP_HI set back to the double 1 - 1e-7 the loss of every
    case that has a log(1 - p) term moves by more than ten times the suite's 1e-4 bar while the gradient does not move by
    a bit. (YOLOv2 and v1.5 take only -t log(p) of a clipped p: the upper bound moves log(hi) by 2e-8, nothing a loss
    comparison could see, which is asserted as such);
  * the gradient of the oracle is exactly 0 on every clipped element outside [lo, hi] and not 0 on lo and hi themselves;
  * ref_head / ref_head_bwd against torch float64 autograd."""
import numpy as np
import pytest
import torch

import saturation_cases as SC
from oracle import losses as OL

BAR = 1e-4


def _oracle(case, yt, yp, dtype=torch.float64):
    p = torch.tensor(yp, dtype=dtype, requires_grad=True)
    loss = SC.oracle_fn(case)(torch.tensor(yt, dtype=dtype), p)
    loss.backward()
    return loss.item(), p.grad.detach().double().numpy()


def test_edge_values_are_the_neighbours_of_the_float32_bounds():
    e = SC.EDGE_P
    assert e.dtype == np.float32 and len(set(e.tolist())) == 10 and np.all(np.diff(e) > 0)
    assert float(e[3]) == OL.CLIP_LO and float(e[7]) == OL.CLIP_HI
    assert e[2] < np.float32(OL.CLIP_LO) < e[4] and e[6] < np.float32(OL.CLIP_HI) < e[8] < e[9] == 1
    assert OL.CLIP_LO > OL.EPSILON and OL.CLIP_HI < 1 - OL.EPSILON       # the float32 roundings, not the doubles


@pytest.mark.parametrize("case", SC.CLIP_CASES, ids=lambda c: c.name)
def test_clip_case_holds_every_edge_value_in_every_kind_of_cell(case):
    yt, yp = SC.clip_inputs(case)
    vals, kinds, chans, _ = SC.clip_channels(case, yt, yp)
    want_kinds = ["resp", "nonresp", "background"] + ([] if case.version == 1 else ["ignored"]) \
        + (["raised"] if case.kw.get("truth_thresh", 1.0) < 1 else [])
    for kname in want_kinds:
        k = SC.KINDS.index(kname)
        groups = [("conf", chans == "conf")]
        if case.version == 1:
            if kname == "resp":
                groups += [("cls_true", chans == "cls_true"), ("cls_wrong", chans == "cls_wrong")]
            elif kname == "background":
                groups += [("cls", chans != "conf")]
        elif kname in ("resp", "raised"):
            groups += [("cls_true", chans == "cls_true")] + ([("cls_wrong", chans == "cls_wrong")] if case.C > 1 else [])
        else:
            groups += [("cls", chans != "conf")]
        for gname, sel in groups:
            for i, e in enumerate(SC.EDGE_P):
                n = int(((kinds == k) & sel & (vals.view(np.uint32) == e.view(np.uint32))).sum())
                assert n >= 1, f"{case.name}: no {SC.EDGE_NAMES[i]} on a {gname} channel of a {kname} anchor"
    if case.version == 2:
        rows = SC.box_view(case, yp)[..., 5:].astype(np.float64).sum(-1)
        assert np.abs(rows - 1).max() < 2e-7


@pytest.mark.parametrize("case", SC.CLIP_CASES + SC.WIDTH_CASES + SC.CHAIN_CASES, ids=lambda c: c.name)
def test_decisions_do_not_depend_on_the_precision(case):
    if case in SC.CLIP_CASES:
        yt, yp = SC.clip_inputs(case)
    elif case in SC.WIDTH_CASES:
        yt, yp = SC.width_inputs(case)
    else:
        yt, t = SC.chain_inputs(case)
        D = t.shape[-1]
        y = SC.join_kinds(SC.ref_head(t.reshape(-1, D), case.version, case.A, case.C, case.anchors), case.version, case.A, case.C)
        yp = y.astype(np.float32).reshape(t.shape)
    truth = case.kw.get("truth_thresh", 1.0)
    k32, i32 = SC.cell_kinds(case, yt, yp, torch.float32)
    k64, i64 = SC.cell_kinds(case, yt, yp, torch.float64)
    assert np.array_equal(k32, k64)
    assert torch.equal(SC.PC.decisions_of(i32, SC.IGNORE, truth), SC.PC.decisions_of(i64, SC.IGNORE, truth))
    assert float((i64 - SC.IGNORE).abs().min()) >= 1e-6 and float((i64 - truth).abs().min()) >= 1e-6
    assert float((i64 - 0.5).abs().min()) >= 1e-6                 # the recall threshold of the metrics
    # the responsible anchor of an object cell wins by more than rounding -- or every IoU of the cell is exactly 0 in both
    # precisions (boxes thinner than the spacing of the numbers at their centre), where both pick anchor 0
    obj = torch.tensor(yt[..., 4].reshape(-1) > 0)
    top = torch.topk(i64[obj], 2, dim=1).values
    zero = (i64[obj] == 0).all(1) & (i32[obj] == 0).all(1)
    assert bool((zero | ((top[:, 0] - top[:, 1]) > 1e-5 * top[:, 0])).all())


@pytest.mark.parametrize("case", SC.WIDTH_CASES, ids=lambda c: c.name)
def test_width_case_holds_every_width(case):
    yt, yp = SC.width_inputs(case)
    kind, _ = SC.cell_kinds(case, yt, yp)
    wh = SC.box_view(case, yp)[..., 2:4]
    if case.version == 1:
        want = [np.full((case.A, 2), v, dtype=np.float32) for v in SC.WIDTH_P_V1]
    else:
        want = [(np.exp(t) * np.array(case.anchors, dtype=np.float64)).astype(np.float32) for t in SC.WIDTH_T]
    for k in (0, 3):                                   # on a responsible anchor and in a background cell
        for wv in want:                                # [A, 2]: one width value on every anchor's w and h
            hit = (wh == wv.reshape(1, 1, 1, case.A, 2)).any(-1)
            assert int((hit & (kind == k)).sum()) >= 1, (case.name, SC.KINDS[k], wv[0])
    an = 1.0 if case.version == 1 else np.array(case.anchors).min()
    tiny = (yt[..., 2] > 0) & (yt[..., 2] / an < 1e-7)
    assert int(tiny.sum()) == 1


@pytest.mark.parametrize("case", SC.CLIP_CASES + SC.WIDTH_CASES, ids=lambda c: c.name)
def test_the_reference_in_float32_is_finite_on_the_case(case):
    yt, yp = SC.clip_inputs(case) if case in SC.CLIP_CASES else SC.width_inputs(case)
    loss, grad = _oracle(case, yt, yp, torch.float32)
    loss64, grad64 = _oracle(case, yt, yp)
    print(f"SATURATION_F32 {case.name}: float32 oracle {loss:.6g}, float64 {loss64:.6g}, largest gradient {np.abs(grad64).max():.3g}")
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert np.isfinite(loss64) and np.isfinite(grad64).all() and np.abs(grad64).max() < 3e38


@pytest.mark.parametrize("case", SC.CLIP_CASES, ids=lambda c: c.name)
def test_clip_case_tells_the_two_upper_bounds_apart(case, monkeypatch):
    yt, yp = SC.clip_inputs(case)
    new, gnew = _oracle(case, yt, yp)
    monkeypatch.setattr(OL, "CLIP_HI", 1 - 1e-7)
    old, gold = _oracle(case, yt, yp)
    rel = abs(old - new) / max(abs(new), 1.0)
    print(f"SATURATION_BOUNDS {case.name}: float32 bound {new:.6f}, float64 bound {old:.6f}, relative difference {rel:.3e}")
    assert np.array_equal(gold.view(np.uint64), gnew.view(np.uint64))        # both bounds mask the same elements
    if SC.HAS_LOG_1MP(case):
        assert rel > 10 * BAR
    else:
        assert rel < 1e-6        # -t log(p) alone: log(0.99999988) against log(0.9999999)


@pytest.mark.parametrize("case", SC.CLIP_CASES, ids=lambda c: c.name)
def test_gradient_mask_of_the_oracle(case):
    yt, yp = SC.clip_inputs(case)
    _, grad = _oracle(case, yt, yp)
    vals, kinds, chans, index = SC.clip_channels(case, yt, yp)
    g = grad.reshape(-1)[index]
    clipped = (chans != "conf") | SC.CONF_IS_CLIPPED(case)
    outside = clipped & ((vals < SC.LO) | (vals > SC.HI))
    assert int(outside.sum()) > 0 and np.all(g[outside] == 0.0)
    seen = 0
    for k in range(len(SC.KINDS)):
        for ch in ("conf", "cls_true", "cls_wrong"):
            if not SC.has_loss_term(case, k, ch):
                continue
            sel = clipped & (kinds == k) & (chans == ch) & ((vals == SC.LO) | (vals == SC.HI))
            seen += int(sel.sum())
            assert np.all(g[sel] != 0.0), (case.name, SC.KINDS[k], ch)
    assert seen > 0


@pytest.mark.parametrize("version,A,C", [(3, 3, 3), (4, 3, 1), (2, 5, 3), (1, 2, 3)])
def test_ref_head_against_autograd(version, A, C):
    g = torch.Generator().manual_seed(version)
    D = 5 * A + C if version == 1 else A * (5 + C)
    P = 7
    t = torch.randn(P, D, generator=g, dtype=torch.float64).requires_grad_(True)
    anchors = (torch.rand(A, 2, generator=g, dtype=torch.float64) + 0.1)
    if version == 1:
        y = torch.cat([torch.sigmoid(t[:, :5 * A]), torch.softmax(t[:, 5 * A:], dim=-1)], dim=-1)
    else:
        tt = t.reshape(P, A, 5 + C)
        cls = torch.softmax(tt[..., 5:], dim=-1) if version == 2 else torch.sigmoid(tt[..., 5:])
        y = torch.cat([torch.sigmoid(tt[..., 0:2]), torch.exp(tt[..., 2:4]) * anchors, torch.sigmoid(tt[..., 4:5]), cls],
                      dim=-1).reshape(P, D)
    dy = torch.randn(P, D, generator=g, dtype=torch.float64)
    y.backward(dy)
    ref = SC.ref_head(t.detach().numpy(), version, A, C, anchors.numpy())
    assert set(ref) == {"xy", "wh", "conf", "cls"}
    got = SC.join_kinds(ref, version, A, C)
    assert np.abs(got - y.detach().numpy()).max() < 1e-14
    bwd = SC.join_kinds(SC.ref_head_bwd(y.detach().numpy(), dy.numpy(), version, A, C), version, A, C)
    assert np.abs(bwd - t.grad.numpy()).max() < 1e-13


def test_logit_table():
    assert sorted(set(np.abs(SC.LOGITS).tolist())) == [0, 1, 8, 15, 18, 30, 88, 89, 104, 200]
    for version, A, C in ((3, 3, 3), (2, 5, 3), (1, 2, 3)):
        t = SC.head_logits(version, A, C)
        cols = SC.head_columns(version, A, C)
        for k in ("xy", "conf", "cls") + (("wh",) if version == 1 else ()):
            for d in cols[k]:
                assert set(t[:SC.NL, d].view(np.uint32).tolist()) == set(SC.LOGITS.view(np.uint32).tolist())
        if version != 1:
            for d in cols["wh"]:
                assert set(t[:, d].tolist()) == set(np.float32(SC.WIDTH_T).tolist())
    for A, C in ((4, 3), (3, 80), (5, 3)):
        b = SC.head_bias(A, C)
        cols = SC.head_columns(3, A, C)
        sig = np.concatenate([cols["xy"], cols["conf"], cols["cls"]])
        assert set(b[sig].view(np.uint32).tolist()) == set(SC.LOGITS.view(np.uint32).tolist())
