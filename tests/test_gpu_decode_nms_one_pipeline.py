"""csrc/decode_nms.hip has ONE decode and ONE NMS pipeline with two front ends: the single-image entry points
(yolo_decode_level(_f64), yolo_nms, yolo_nms_select) are the batched ones (yolo_decode_batch_*, yolo_nms_batch_*) with
B = 1. Pinned here byte for byte, on rows and levels drawn on the CPU with fixed seeds; the oracle (oracle/tools.py) says
what both must give, so that "equal" cannot mean "equally wrong".

decode: a level of 13 x 13 x 3 boxes x 5 classes = 2 535 candidate slots (two workgroups of 2 048, the second partly
filled), then one of 7 x 7 (735 slots) behind it: the single path appends it through the carry-in count. The last axis is
3 * (5 + 5) = 30 for version 3 and 5 * 3 + 5 = 20 for version 1 (the version-1 layout shares the class columns of a cell).
NMS: 300 rows in a handful of classes, the first of them with about half the rows (three 64-row tiles of the bit matrix);
class_num 3, 1 100 (past one 1 024-segment step of the segment scans) and 3 000 (past NMS_LDS_CLASSES = 2 048: global
counters); the class ids in use straddle those limits."""
import functools

import numpy as np
import pytest
import torch

from oracle import tools as OT

pytestmark = pytest.mark.gpu

DEC_THR = 0.375         # the same number in float32 and float64; P(u * v >= t) = 1 - t + t ln t = 0.257 for uniform u, v
A, C = 3, 5
NMS_THR, CONF_THR, SIGMA = 0.45, 0.5, 0.5
CLASS_IDS = {3: (0, 1, 2), 1100: (1099, 0, 1023, 1024), 3000: (2048, 5, 2047, 2999)}     # the first one holds half the rows


# ---- decode ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def levels(version, dtype):
    rng = np.random.default_rng(41)
    D = 5 * A + C if version == 1 else A * (5 + C)
    return tuple(rng.random((1, g, g, D)).astype(dtype) for g in (13, 7))


def _products(lv, version):
    """conf * prob of every candidate slot, in the level's own type"""
    if version == 1:
        conf = lv[..., :5 * A].reshape(*lv.shape[:3], A, 5)[..., 4]
        return conf[..., :, None] * lv[..., None, 5 * A:]
    t = lv.reshape(*lv.shape[:3], A, 5 + C)
    return t[..., 4:5] * t[..., 5:]


@functools.lru_cache(maxsize=None)
def oracle_decoded(version, dtype):
    lv = levels(version, dtype)
    return np.asarray(OT.decode(*[a[0] for a in lv], class_num=C, threshold=DEC_THR, version=version)).reshape(-1, 7)


def _decode_single(lv, version, max_rows, capacity):
    """ops.decode_level level by level into one buffer of `capacity` rows filled with -7 -> (buffer, count)"""
    from tf2_yolo_amd import ops
    rows = torch.full((capacity, 7), -7.0, device="cuda", dtype=torch.float64)
    count = torch.zeros(1, device="cuda", dtype=torch.int32)
    for a in lv:
        t = torch.from_numpy(a[0]).cuda()
        ws = torch.empty(ops.decode_workspace_bytes(t.shape[0], t.shape[1], A, C), device="cuda", dtype=torch.uint8)
        ops.decode_level(t, A, C, version, DEC_THR, rows, max_rows, count, ws)
    return rows.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("version", [1, 3])
def test_decode_level_by_level_equals_decode_batch(version, dtype):
    from tf2_yolo_amd import ops
    lv = levels(version, dtype)
    assert [a.shape[1] * a.shape[2] * A * C for a in lv] == [2535, 735]
    passing = [int((_products(a, version) >= dtype(DEC_THR)).sum()) for a in lv]
    assert all(0.2 * s < p < 0.3 * s for p, s in zip(passing, (2535, 735))), passing     # roughly a quarter
    want = oracle_decoded(version, dtype)
    n = sum(passing)
    assert want.shape == (n, 7)

    rows_b, img_off = ops.decode_batch([torch.from_numpy(a).cuda() for a in lv], [A, A], C, version, [DEC_THR, DEC_THR])
    assert img_off.cpu().tolist() == [0, n]
    rows_b = rows_b.cpu().numpy()
    rows_s, count = _decode_single(lv, version, n, n)
    assert count == n
    assert rows_s.tobytes() == rows_b.tobytes()
    assert np.array_equal(rows_b, want)

    # max_rows below the count: the first max_rows rows are written, nothing behind them, and the full count is reported --
    # cut inside the second level, then inside the first (the second level then writes nothing at all)
    for m in (passing[0] + 10, passing[0] // 2):
        cut, count = _decode_single(lv, version, m, n)
        assert count == n
        assert cut[:m].tobytes() == rows_b[:m].tobytes()
        assert np.all(cut[m:] == -7.0)


# ---- NMS -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nms_rows(class_num):
    rng = np.random.default_rng(43)
    n, ids = 300, CLASS_IDS[class_num]
    r = np.empty((n, 7))
    r[:, 0:2] = rng.random((n, 2))
    r[:, 2:4] = 0.2 + 0.4 * rng.random((n, 2))
    r[:, 4] = 0.8 + 0.2 * rng.random(n)
    r[:, 5] = rng.choice(ids, size=n, p=[0.5] + [0.5 / (len(ids) - 1)] * (len(ids) - 1))
    r[:, 6] = 0.7 + 0.3 * rng.random(n)
    r[7, 5], r[50, 5], r[120, 5], r[200, 5] = -2, class_num, class_num + 5000, -1          # not classes: never kept
    r[40] = r[20]                                   # one exact score tie, between two boxes of which one suppresses the other
    r[40, 0] += 0.01
    r[20, 5] = r[40, 5] = ids[0]
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_keep(class_num, mode):
    from tf2_yolo_amd import _lib
    r = nms_rows(class_num)
    if mode == _lib.NMS_SOFT:
        return OT.soft_nms_keep(r, class_num, NMS_THR, CONF_THR, SIGMA)
    return OT.nms_keep(r, class_num, NMS_THR, 2 if mode == _lib.NMS_DIOU else 1)


def _nms_args(mode):
    return (mode, NMS_THR, CONF_THR, SIGMA)


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("mode_name", ["hard", "soft", "diou"])
@pytest.mark.parametrize("class_num", [3, 1100, 3000])
def test_nms_select_equals_batch_select_of_one_image(class_num, mode_name, walk):
    from tf2_yolo_amd import _lib, ops
    mode = {"hard": _lib.NMS_HARD, "soft": _lib.NMS_SOFT, "diou": _lib.NMS_DIOU}[mode_name]
    r = nms_rows(class_num)
    n = r.shape[0]
    valid = (r[:, 5] >= 0) & (r[:, 5] < class_num)
    assert valid.sum() == n - 4 and (r[:, 5] < 0).any() and (r[:, 5] >= class_num).any()
    assert r[20, 4] * r[20, 6] == r[40, 4] * r[40, 6] and r[20, 5] == r[40, 5]
    assert OT.cal_iou(r[20:21, :5], r[40:41, :5])[0] >= NMS_THR
    want_keep = oracle_keep(class_num, mode)
    assert not want_keep[~valid].any() and 0 < want_keep.sum() < valid.sum()          # rows are kept, rows are removed
    want = OT._gather_by_class(r, want_keep, class_num)

    rows = torch.from_numpy(r.copy()).cuda()
    img_off = torch.tensor([0, n], device="cuda", dtype=torch.int32)
    try:
        ops.set_option(ops.OPT_NMS_WALK, walk)
        single = ops.nms_select(rows, class_num, *_nms_args(mode)).cpu().numpy()
        batch, kept_off = ops.nms_batch_select(rows, img_off, class_num, *_nms_args(mode))
        keep = ops.nms_keep(rows, class_num, *_nms_args(mode)).cpu().numpy()
    finally:
        ops.reset_options()
    m = single.shape[0]
    assert list(kept_off) == [0, m]
    assert single.tobytes() == batch.cpu().numpy().tobytes()
    assert np.array_equal(keep.astype(bool), want_keep)
    assert np.array_equal(single, want)


def test_no_rows():
    from tf2_yolo_amd import _lib, ops
    rows = torch.from_numpy(nms_rows(3).copy()).cuda()[:0]
    assert tuple(ops.nms_select(rows, 3, *_nms_args(_lib.NMS_HARD)).shape) == (0, 7)
    out, kept_off = ops.nms_batch_select(rows, torch.zeros(2, device="cuda", dtype=torch.int32), 3, *_nms_args(_lib.NMS_HARD))
    assert tuple(out.shape) == (0, 7) and list(kept_off) == [0, 0]


@pytest.mark.parametrize("mode_name", ["hard", "soft"])
def test_one_image_without_a_matrix_buffer(mode_name):
    """yolo_nms_batch_select with B = 1, mask = NULL, mask_words = 0 although the segment scan asks for words: every
    segment goes to the walk / tiled kernels, and the rows are those of yolo_nms_select (bit matrices in its workspace)"""
    from tf2_yolo_amd import _lib, ops
    mode = {"hard": _lib.NMS_HARD, "soft": _lib.NMS_SOFT}[mode_name]
    class_num = 3
    r = nms_rows(class_num)
    n, lib = r.shape[0], _lib.load()
    assert (r[:, 5] == 0).sum() > 128            # a segment of three tiles: 3 words a row
    rows = torch.from_numpy(r.copy()).cuda()
    img_off = torch.tensor([0, n], device="cuda", dtype=torch.int32)
    nbytes = int(lib.yolo_nms_batch_workspace_bytes(n, 1, class_num))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    words = torch.zeros(1, device="cuda", dtype=torch.int64)
    _lib.check(lib.yolo_nms_batch_prepare(ops._p(rows), n, ops._p(img_off), 1, class_num, ops._p(words), ops._p(ws), nbytes,
                                          ops._stream()), "yolo_nms_batch_prepare")
    assert int(words.item()) >= 128 * 3
    keep = torch.empty(n, device="cuda", dtype=torch.uint8)
    out = torch.empty((n, 7), device="cuda", dtype=torch.float64)
    kept_off = torch.empty(2, device="cuda", dtype=torch.int32)
    _lib.check(lib.yolo_nms_batch_select(ops._p(rows), n, 1, class_num, mode, NMS_THR, CONF_THR, SIGMA, None, 0, ops._p(keep),
                                         ops._p(out), ops._p(kept_off), ops._p(ws), nbytes, ops._stream()),
               "yolo_nms_batch_select")
    single = ops.nms_select(rows, class_num, *_nms_args(mode)).cpu().numpy()
    offs = kept_off.cpu().tolist()
    assert offs == [0, single.shape[0]]
    assert out[:offs[1]].cpu().numpy().tobytes() == single.tobytes()
    assert np.array_equal(single, OT._gather_by_class(r, oracle_keep(class_num, mode), class_num))
