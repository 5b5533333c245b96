"""Case tables of the saturation tests (tests/test_gpu_saturation.py), GPU-free: predictions AT the clip bounds of the
losses, widths at the ends of the finite range, head logits where sigmoid / softmax / exp saturate, and float64 NumPy
references of the head. Nothing here imports the library or touches a device; tests/test_saturation_cases_cpu.py checks
that every case contains what it is meant to contain and that the reference itself is finite on it.

The reference clips confidences and class probabilities with tf.clip_by_value(p, 1e-7, 1 - 1e-7) on float32 tensors:
lo = float32(1e-7), hi = float32(1 - 1e-7) = 0.99999988 (oracle/losses.py: CLIP_LO / CLIP_HI). A trained network is out
there all the time: sigmoid(t) is exactly 1.0f for t > 16.6 and below lo for t < -16.1.

  clip cases   every confidence and class probability is one of EDGE_P, cyclically, so that every edge value occurs in
               every kind of cell the loss distinguishes (KINDS); boxes stay ordinary (the decisions must not hang on the
               precision of an IoU)
  width cases  kept apart, their gradients ~ 1 / w are 30 orders larger: w, h = exp(t) anchor for t in WIDTH_T (v1: the
               raw p of WIDTH_P_V1), and one true width below 1e-7 anchor
  head table   LOGITS on the sigmoid / softmax channels, WIDTH_T on the exp channels, three special softmax rows
  chain        logits -> head -> loss -> gradient -> head backward: box logits ordinary, confidence / class logits LOGITS
               (a softmax row: one class from LOGITS, the others ordinary)
"""
from collections import namedtuple

import numpy as np

import past_cap_cases as PC

F = np.float32
LO, HI = F(1e-7), F(1 - 1e-7)


def pred(x):
    return np.nextafter(F(x), F(-1))


def succ(x):
    return np.nextafter(F(x), F(2))


EDGE_P = np.array([0.0, np.nextafter(F(0), F(1)), pred(LO), LO, succ(LO), 0.5, pred(HI), HI, succ(HI), 1.0], dtype=F)
EDGE_NAMES = ("0", "subnormal", "pred(lo)", "lo", "succ(lo)", "0.5", "pred(hi)", "hi", "succ(hi)", "1")
assert EDGE_P[8] == F(0.99999994) and succ(EDGE_P[8]) == F(1) and 0 < EDGE_P[1] < F(1.2e-38)
NE = len(EDGE_P)

# the finite range of the widths: exp(-80) anchor = 1.8e-35 anchor is a normal float32 and 0.02 log(w / anchor) / w, the
# regulariser's gradient, stays below 1e37; exp(9) anchor = 8103 anchor squares to an area far from overflow
WIDTH_T = (-80.0, -40.0, -16.2, 0.0, 4.0, 9.0)
WIDTH_P_V1 = np.array([0.0, pred(LO), LO, succ(LO), 0.25, 1.0], dtype=F)
TINY_TRUE_W = F(1e-9)                       # true width / anchor < 1e-7 for every anchor below (anchors < 1)

_L = (0.0, 1.0, 8.0, 15.0, 18.0, 30.0, 88.0, 89.0, 104.0, 200.0)
LOGITS = np.array(sorted([-v for v in _L] + list(_L), key=lambda v: (v, np.signbit(v) == 0)), dtype=F)   # -200 .. -0, +0 .. 200
NL = len(LOGITS)
assert NL == 20 and np.signbit(LOGITS[9]) and not np.signbit(LOGITS[10])

ANCH3, ANCH5 = PC.ANCH9[:3], PC.ANCH5
IGNORE = 0.6
BW, LW4, LW3 = 0.7, [1.5, 1.2, 5, 2.0], [1.5, 5, 2.0]
KINDS = ("resp", "nonresp", "ignored", "background", "raised")

# kw: truth_thresh / label_smooth (shared by ops.make_loss_cfg and the oracle); focal, gamma: v3's switch, the exponent
SatCase = namedtuple("SatCase", "name version N g A C anchors seed kw focal gamma")

CLIP_CASES = [
    SatCase("v3", 3, 3, (8, 6), 3, 3, ANCH3, 1, {}, False, 2),
    SatCase("v3-focal-g2", 3, 3, (6, 8), 3, 3, ANCH3, 2, {}, True, 2),
    SatCase("v3-focal-g1.5-c1", 3, 3, (8, 6), 3, 1, ANCH3, 3, {}, True, 1.5),
    SatCase("v4-c1", 4, 3, (7, 6), 3, 1, ANCH3, 4, {"label_smooth": 0.0}, False, 2),
    SatCase("v4-smooth", 4, 3, (8, 6), 3, 3, ANCH3, 5, {"label_smooth": 0.1}, False, 2),
    SatCase("v4-truth", 4, 3, (8, 6), 3, 3, ANCH3, 6, {"truth_thresh": 0.7}, False, 2),
    SatCase("v2", 2, 3, (8, 6), 5, 3, ANCH5, 7, {}, False, 2),
    SatCase("v1", 1, 3, (8, 6), 2, 3, None, 8, {}, False, 2),
]
WIDTH_CASES = [
    SatCase("w-v3", 3, 3, (8, 6), 3, 3, ANCH3, 11, {}, False, 2),
    SatCase("w-v4", 4, 3, (6, 8), 3, 3, ANCH3, 12, {}, False, 2),
    SatCase("w-v2", 2, 3, (8, 6), 5, 3, ANCH5, 13, {}, False, 2),
    SatCase("w-v1", 1, 3, (8, 6), 2, 3, None, 14, {}, False, 2),
]
CHAIN_CASES = [
    SatCase("chain-v3-focal", 3, 3, (8, 6), 3, 3, ANCH3, 21, {}, True, 2),
    SatCase("chain-v4-truth", 4, 3, (8, 6), 3, 3, ANCH3, 22, {"truth_thresh": 0.7}, False, 2),
    SatCase("chain-v2", 2, 3, (8, 6), 5, 3, ANCH5, 23, {}, False, 2),
    SatCase("chain-v1", 1, 3, (8, 6), 2, 3, None, 24, {}, False, 2),
]
# which channels of a version go through clip_by_value in the loss
CONF_IS_CLIPPED = lambda c: c.version == 4 or (c.version == 3 and c.focal)   # noqa: E731
# the upper bound enters a loss only through log(1 - p): v2 and v1.5 have -t log(p) alone
HAS_LOG_1MP = lambda c: c.version in (3, 4)   # noqa: E731


def oracle_fn(case, parts=False):
    """the oracle's closure of a case (weights BW / LW4 / LW3)"""
    from oracle import losses as OL
    g, A, C, v = case.g, case.A, case.C, case.version
    if v == 3:
        return OL.wrap_yolo_loss_v3(g, A, C, anchors=case.anchors, binary_weight=BW, loss_weight=LW4, ignore_thresh=IGNORE,
                                    use_focal_loss=case.focal, focal_loss_gamma=case.gamma, parts=parts)
    if v == 2:
        return OL.wrap_yolo_loss_v2(g, A, C, case.anchors, binary_weight=BW, loss_weight=LW4, ignore_thresh=IGNORE)
    if v == 4:
        return OL.wrap_yolo_loss_v4(g, A, C, case.anchors, binary_weight=BW, loss_weight=LW3, wh_reg_weight=0.01,
                                    ignore_thresh=IGNORE, focal_loss_gamma=case.gamma, **case.kw)
    return OL.wrap_yolo_loss_v1(g, A, C, binary_weight=BW, loss_weight=LW4)


def cfg_args(case):
    """positional and keyword arguments of ops.make_loss_cfg for the same loss"""
    return ((case.version, case.N, case.g[0], case.g[1], case.A, case.C, case.anchors),
            dict(binary_weight=BW, loss_weight=LW3 if case.version == 4 else LW4, ignore_thresh=IGNORE, wh_reg_weight=0.01,
                 use_focal_loss=case.focal, focal_gamma=case.gamma, **case.kw))


def _base(case):
    """make_case of tests/test_gpu_loss.py with 30 % object cells; in every second object cell anchors 0, 1, 2 sit on the
    truth with the extents scaled by 1.01, 1.05, 1.2: IoU 0.98 (responsible), 0.91 (ignored; raised by a truth_thresh of
    0.7) and 0.69 (ignored)"""
    from test_gpu_loss import make_case
    yt, yp = make_case(case.N, case.g, case.A, case.C, case.anchors, case.seed, v1=case.version == 1, obj_frac=0.3)
    if case.version != 1:
        yp5 = yp.reshape(case.N, *case.g, case.A, 5 + case.C)
        for i, (n, y, x) in enumerate(np.argwhere(yt[..., 4] > 0)):
            if i % 2 == 0:
                for b, s in ((0, 1.01), (1, 1.05), (2, 1.2)):
                    yp5[n, y, x, b, 0:2] = yt[n, y, x, 0:2]
                    yp5[n, y, x, b, 2:4] = yt[n, y, x, 2:4] * F(s)
    return yt, yp


def box_view(case, yp):
    """[N, gh, gw, A, 5 (+ C)] view of the per-anchor channels of y_pred"""
    if case.version == 1:
        return yp[..., :5 * case.A].reshape(case.N, *case.g, case.A, 5)
    return yp.reshape(case.N, *case.g, case.A, 5 + case.C)


def cell_kinds(case, yt, yp, dtype=None):
    """[N, gh, gw, A] indices into KINDS, from the IoUs of past_cap_cases.loss_case_ious and the decisions of
    past_cap_cases.decisions_of; also the IoUs [cells, A]"""
    import torch
    truth = case.kw.get("truth_thresh", 1.0)
    iou, t4 = PC.loss_case_ious(case, dtype or torch.float64, inputs=(yt, yp))
    dec = PC.decisions_of(iou, IGNORE, truth)
    A = case.A
    ar = torch.arange(A)
    obj = (t4 > 0).unsqueeze(1)
    resp = obj & (dec[:, 0:1] == ar)
    raised = ((dec[:, 1:2] >> (16 + ar)) & 1).bool() & ~resp if (case.version == 4 and truth < 1) else torch.zeros_like(resp)
    ign = ~((dec[:, 1:2] >> ar) & 1).bool() & ~resp & ~raised if case.version != 1 else torch.zeros_like(resp)
    kind = torch.full(resp.shape, 3, dtype=torch.long)                       # background
    kind[obj.expand_as(resp)] = 1
    kind[ign] = 2
    kind[raised] = 4
    kind[resp] = 0
    return kind.reshape(case.N, *case.g, A).numpy(), iou


def clip_inputs(case):
    """(y_true, y_pred): _base with every confidence and class probability overwritten, cyclically per kind of cell, by
    EDGE_P. v2: the class rows sum to 1 (one edge value, the rest shared evenly) -- they are softmax outputs."""
    yt, yp = _base(case)
    kind, _ = cell_kinds(case, yt, yp)
    v5 = box_view(case, yp)
    C, A = case.C, case.A
    tcls = yt[..., 5:].argmax(-1)
    has = yt[..., 4] > 0
    for k in range(len(KINDS)):
        for r, (n, y, x, b) in enumerate(np.argwhere(kind == k)):
            v5[n, y, x, b, 4] = EDGE_P[r % NE]
            if case.version == 1:
                continue
            row = v5[n, y, x, b, 5:]
            tc = int(tcls[n, y, x])
            if case.version == 2:
                at = (tc + (r % 2)) % C if has[n, y, x] else r % C       # even r: the true class, odd r: a wrong one
                e = EDGE_P[(r // 2) % NE]
                row[:] = (F(1) - e) / F(C - 1)
                row[at] = e
            elif has[n, y, x]:
                j = 0
                for c in range(C):
                    if c == tc:
                        row[c] = EDGE_P[(r + 3) % NE]
                    else:
                        row[c] = EDGE_P[(r + 5 + 3 * j) % NE]
                        j += 1
            else:
                for c in range(C):
                    row[c] = EDGE_P[(r + 3 + 3 * c) % NE]
    if case.version == 1:                 # the class probabilities of a v1.5 cell: one row per cell
        cls = yp[..., 5 * A:]
        for obj in (True, False):
            for r, (n, y, x) in enumerate(np.argwhere(has == obj)):
                tc, j = int(tcls[n, y, x]), 0
                for c in range(C):
                    if obj and c == tc:
                        cls[n, y, x, c] = EDGE_P[(r + 3) % NE]
                    else:
                        cls[n, y, x, c] = EDGE_P[(r + 5 + 3 * j) % NE]
                        j += 1
    return yt, yp


def clip_channels(case, yt, yp):
    """the clip case by element: (values, kind index, channel kind, clipped) as flat arrays over every confidence and class
    element. channel kind: "conf", "cls_true" (class channel of the cell's true class, object cells), "cls_wrong".
    For v1.5 the class row belongs to the cell: its kind is "resp" in an object cell, "background" otherwise."""
    kind, _ = cell_kinds(case, yt, yp)
    v5 = box_view(case, yp)
    C, A = case.C, case.A
    has = yt[..., 4] > 0
    onehot = (yt[..., 5:] > 0) & has[..., None]                           # [N, gh, gw, C]
    vals, kinds, chans, index = [v5[..., 4].reshape(-1)], [kind.reshape(-1)], [np.full(kind.size, "conf", dtype=object)], []
    flat = np.arange(yp.size).reshape(yp.shape)
    index.append(box_view(case, flat)[..., 4].reshape(-1))
    if case.version == 1:
        cls = yp[..., 5 * A:]
        vals.append(cls.reshape(-1))
        kinds.append(np.broadcast_to(np.where(has, 0, 3)[..., None], cls.shape).reshape(-1))
        chans.append(np.where(onehot, "cls_true", "cls_wrong").astype(object).reshape(-1))
        index.append(flat[..., 5 * A:].reshape(-1))
    else:
        cls = v5[..., 5:]
        vals.append(cls.reshape(-1))
        kinds.append(np.broadcast_to(kind[..., None], cls.shape).reshape(-1))
        chans.append(np.broadcast_to(np.where(onehot, "cls_true", "cls_wrong").astype(object)[:, :, :, None, :], cls.shape).reshape(-1))
        index.append(box_view(case, flat)[..., 5:].reshape(-1))
    return (np.concatenate(vals), np.concatenate(kinds), np.concatenate(chans), np.concatenate(index))


def has_loss_term(case, kind, chan):
    """does the loss of `case` depend on a confidence / class element of this kind of cell?"""
    k = KINDS[kind]
    if chan == "conf":
        return k != "ignored"
    if case.version == 1:
        return k == "resp" and chan == "cls_true"
    if k not in ("resp", "raised"):
        return False
    return chan == "cls_true" or case.version in (3, 4)


def channel_kinds(case):
    """channel kind ("xy", "wh", "conf", "cls") of every prediction channel of a cell: array of PD strings"""
    A, C = case.A, case.C
    per = ["xy", "xy", "wh", "wh", "conf"]
    if case.version == 1:
        return np.array(per * A + ["cls"] * C, dtype=object)
    return np.array((per + ["cls"] * C) * A, dtype=object)


# ---- width cases -----------------------------------------------------------------------------------------------------
_PAIRS = [(a, b) for a in WIDTH_T for b in WIDTH_T]
_UNDER = [(-80.0, -80.0), (-80.0, -40.0), (-40.0, -80.0)]      # areas that underflow float32: IoU exactly 0 there
_RESP = [p for p in _PAIRS if p[0] + p[1] >= -76.0]            # areas that are normal float32 numbers


def width_inputs(case):
    """(y_true, y_pred). In object cell i ONE anchor is centred on the truth and walks the pairs (_RESP, or all 36 of
    WIDTH_P_V1 for v1.5) while the other anchors have areas that are exactly 0 in float32 and below 1e-50 in float64
    (_UNDER; v1.5: w = 0 or h = 0), so that anchor is the responsible one in float32 and float64 alike. It is anchor i % A
    -- but anchor 0 where its box is thinner than float32 resolves at its centre (t = -16.2, the v1.5 widths around
    1e-7): there its IoU may round to 0 in one precision only, and a cell of zeros goes to anchor 0 anyway. Background
    cells (every IoU exactly 0) walk all 36 pairs on every anchor. The first object cell has a true width of 1e-9."""
    yt, yp = _base(case)
    v5 = box_view(case, yp)
    A = case.A
    cells = np.argwhere(yt[..., 4] > 0)
    bg = np.argwhere(np.broadcast_to((yt[..., 4] == 0)[..., None], v5.shape[:4]))
    if case.version == 1:
        P = WIDTH_P_V1
        for i, (n, y, x) in enumerate(cells):
            pw, ph = P[i % 6], P[(i // 6 + i) % 6]
            r = i % A if min(pw, ph) == 0 or min(pw, ph) > 0.1 else 0
            for b in range(A):
                v5[n, y, x, b, 2:4] = (pw, ph) if b == r else ((0, P[(i + b) % 6]) if (i + b) % 2 else (P[(i + b) % 6], 0))
            v5[n, y, x, r, 0:2] = yt[n, y, x, 0:2]
        for j, (n, y, x, b) in enumerate(bg):
            v5[n, y, x, b, 2:4] = (P[j % 6], P[(j // 6 + j) % 6])
    else:
        anc = np.array(case.anchors, dtype=np.float64)
        for i, (n, y, x) in enumerate(cells):
            pair = _RESP[i % len(_RESP)]
            r = 0 if -16.2 in pair else i % A
            for b in range(A):
                v5[n, y, x, b, 2:4] = (np.exp(pair if b == r else _UNDER[(i + b) % 3]) * anc[b]).astype(F)
            v5[n, y, x, r, 0:2] = yt[n, y, x, 0:2]
        for j, (n, y, x, b) in enumerate(bg):
            v5[n, y, x, b, 2:4] = (np.exp(_PAIRS[j % 36]) * anc[b]).astype(F)
    n, y, x = cells[0]
    yt[n, y, x, 2] = TINY_TRUE_W
    return yt, yp


# ---- the head ----------------------------------------------------------------------------------------------------------
def head_columns(version, A, C):
    """column indices of a head tensor [P, D] per channel kind. v1.5: D = 5 A + C, all of x, y, w, h, c are sigmoids;
    v2 / v3 / v4: D = A (5 + C), w and h are exp(t) anchor"""
    case = SatCase("", version, 0, (0, 0), A, C, None, 0, {}, False, 2)
    ck = channel_kinds(case)
    return {k: np.nonzero(ck == k)[0] for k in ("xy", "wh", "conf", "cls")}


def is_softmax(version):
    return version in (1, 2)


def head_logits(version, A, C):
    """t float32 [P, D]: rows 0..19 walk LOGITS on every sigmoid / softmax channel (each channel sees every logit) and
    WIDTH_T on the exp channels; the softmax versions get three more rows: one class logit 200 above the rest, all class
    logits equal, all class logits -200"""
    D = 5 * A + C if version == 1 else A * (5 + C)
    P = NL + (3 if is_softmax(version) else 0)
    t = np.zeros((P, D), dtype=F)
    cols = head_columns(version, A, C)
    for p in range(P):
        for d in range(D):
            t[p, d] = LOGITS[(p + 7 * d) % NL]
        if version != 1:
            for i, d in enumerate(cols["wh"]):
                t[p, d] = WIDTH_T[(p + i) % 6]
    if is_softmax(version):
        rows = t[:, cols["cls"]].reshape(P, -1, C)
        rows[NL] = -15.0
        rows[NL, :, C // 2] = 185.0
        rows[NL + 1] = 15.0
        rows[NL + 2] = -200.0
        t[:, cols["cls"]] = rows.reshape(P, -1)
    return t


def head_bias(A, C):
    """the logit table cycled over the A (5 + C) channels of a v2 / v3 / v4 head (the bias of the fused-head test): the
    i-th sigmoid / softmax channel holds LOGITS[i % 20], the j-th exp channel WIDTH_T[j % 6]"""
    cols = head_columns(3, A, C)
    b = np.zeros(A * (5 + C), dtype=F)
    sig = np.sort(np.concatenate([cols["xy"], cols["conf"], cols["cls"]]))
    b[sig] = LOGITS[np.arange(len(sig)) % NL]
    b[cols["wh"]] = np.array(WIDTH_T, dtype=F)[np.arange(2 * A) % 6]
    return b


def _sigmoid(t):
    return 1.0 / (1.0 + np.exp(-t))


def ref_head(t, version, A, C, anchors=None):
    """float64 head activation of t [P, D], per channel kind: {"xy", "wh", "conf", "cls"} -> [P, columns of that kind]"""
    t = np.asarray(t, dtype=np.float64)
    P = t.shape[0]
    cols = head_columns(version, A, C)
    out = {k: _sigmoid(t[:, cols[k]]) for k in ("xy", "conf")}
    if version == 1:
        out["wh"] = _sigmoid(t[:, cols["wh"]])
    else:
        out["wh"] = np.exp(t[:, cols["wh"]]) * np.asarray(anchors, dtype=np.float64).reshape(1, 2 * A)
    tc = t[:, cols["cls"]]
    if is_softmax(version):
        rows = tc.reshape(P, -1, C)
        e = np.exp(rows - rows.max(-1, keepdims=True))
        out["cls"] = (e / e.sum(-1, keepdims=True)).reshape(P, -1)
    else:
        out["cls"] = _sigmoid(tc)
    return out


def ref_head_bwd(y, dy, version, A, C):
    """float64 backward of the head FROM ITS OUTPUT y, as TensorFlow's gradients are: sigmoid dy y (1 - y), exp dy y, softmax
    y (dy - sum(dy y)); per channel kind like ref_head"""
    y, dy = np.asarray(y, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    P = y.shape[0]
    cols = head_columns(version, A, C)
    sg = lambda k: dy[:, cols[k]] * y[:, cols[k]] * (1.0 - y[:, cols[k]])   # noqa: E731
    out = {"xy": sg("xy"), "conf": sg("conf")}
    out["wh"] = sg("wh") if version == 1 else dy[:, cols["wh"]] * y[:, cols["wh"]]
    if is_softmax(version):
        yr, gr = y[:, cols["cls"]].reshape(P, -1, C), dy[:, cols["cls"]].reshape(P, -1, C)
        out["cls"] = (yr * (gr - (gr * yr).sum(-1, keepdims=True))).reshape(P, -1)
    else:
        out["cls"] = sg("cls")
    return out


def join_kinds(parts, version, A, C):
    """[P, D] from the per-kind arrays of ref_head / ref_head_bwd"""
    cols = head_columns(version, A, C)
    P = parts["xy"].shape[0]
    out = np.zeros((P, sum(len(c) for c in cols.values())))
    for k, c in cols.items():
        out[:, c] = parts[k]
    return out


def chain_inputs(case):
    """(y_true, t): logits [N, gh, gw, PD] whose head output is _base's boxes (ordinary: logit / log of them) and whose
    confidence and class logits walk LOGITS"""
    yt, yp = _base(case)
    v5 = box_view(case, yp).astype(np.float64)
    t = np.zeros(yp.shape, dtype=F)
    t5 = box_view(case, t)
    logit = lambda p: np.log(p / (1 - p))   # noqa: E731
    t5[..., 0:2] = logit(np.clip(v5[..., 0:2], 1e-3, 1 - 1e-3))
    if case.version == 1:
        t5[..., 2:4] = logit(np.clip(v5[..., 2:4], 1e-3, 1 - 1e-3))
    else:
        t5[..., 2:4] = np.log(v5[..., 2:4] / np.array(case.anchors, dtype=np.float64))
    n = int(np.prod(t5.shape[:4]))
    r = np.arange(n).reshape(t5.shape[:4])
    t5[..., 4] = LOGITS[r % NL]
    C = case.C
    # sigmoid classes: every class logit walks LOGITS. softmax rows: ONE class walks LOGITS, the others stay at
    # -0.5, 0, 0.5, ... -- rows of table logits alone are one-hot to the last bit and leave no class gradient to compare
    rows = np.arange(int(np.prod(t.shape[:3]))).reshape(t.shape[:3]) if case.version == 1 else r
    for c in range(C):
        if is_softmax(case.version):
            v = np.where(rows % C == c, LOGITS[(3 * rows + 5) % NL], F(0.5 * (c - 1)))
        else:
            v = LOGITS[(3 * rows + 7 * c + 5) % NL]
        if case.version == 1:
            t[..., 5 * case.A + c] = v
        else:
            t5[..., 5 + c] = v
    return yt, t
