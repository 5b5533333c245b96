"""tools.detect_batch / Model.detect: decode + NMS of a whole batch on the device (csrc/decode_nms.hip: the batched decode
kernels, nms_prepare_batch_kernel and the segment scans in front of the per-image NMS kernels).

Expected values: oracle/tools.py per image -- decode of the image's slices, then nms / soft_nms / nms(iou_mode=2) --
compared bit for bit (np.array_equal on float64, no tolerance). The inputs of those cases are drawn so that no two
conf * prob products inside one (image, class) are equal (asserted), because the oracle's order of exact ties is its own.
A second assertion compares with the per-image device functions (tools.decode, tools.nms, tools.soft_nms), which also
covers exact ties. Every case first proves on the oracle's output that it is not vacuous: rows are kept in at least two
images, hard NMS removes rows in at least two images, and only the deliberately empty images are empty."""
import functools

import numpy as np
import pytest
import torch

from oracle import tools as OT

pytestmark = pytest.mark.gpu

THR, NMS_THR, SIGMA = 0.5, 0.45, 0.5     # 0.5 is the same number in float32 and float64


# ---- inputs (CPU only) ---------------------------------------------------------------------------------------------
def _rand_level(rng, B, gh, gw, A, C, version, dtype):
    """uniform [0, 1) entries (about 15 % of the conf * prob products pass 0.5), widths and heights in [0.2, 0.6)"""
    if version == 1:
        box = rng.random((B, gh, gw, A, 5))
        box[..., 2:4] = 0.2 + 0.4 * rng.random((B, gh, gw, A, 2))
        prob = rng.random((B, gh, gw, C))
        return np.concatenate([box.reshape(B, gh, gw, 5 * A), prob], axis=-1).astype(dtype)
    t = rng.random((B, gh, gw, A, 5 + C))
    t[..., 2:4] = 0.2 + 0.4 * rng.random((B, gh, gw, A, 2))
    return t.reshape(B, gh, gw, A * (5 + C)).astype(dtype)


def _case(levels, C, version, empty=(), degenerate=False, ties=False):
    return {"levels": levels, "C": C, "version": version, "empty": set(empty), "degenerate": degenerate, "ties": ties}


def _boundaries(dtype):
    # 1 440 slots per image on the finest level: image boundaries fall inside the 2 048-candidate blocks of a flat grid
    rng = np.random.default_rng(11)
    return _case([_rand_level(rng, 3, gh, gw, 3, 5, 3, dtype) for gh, gw in ((2, 3), (4, 6), (8, 12))], 5, 3)


def _empty_middle():
    # image 1 has no candidate at all; every candidate of image 2 is of class 3
    rng = np.random.default_rng(12)
    t = _rand_level(rng, 3, 6, 8, 3, 5, 3, np.float32).reshape(3, 6, 8, 3, 10)
    t[1, ..., 4] = 0
    keep = t[2, ..., 5 + 3].copy()
    t[2, ..., 5:] = 0
    t[2, ..., 5 + 3] = keep
    return _case([t.reshape(3, 6, 8, 30)], 5, 3, empty={1})


def _all_empty():
    rng = np.random.default_rng(13)
    lv = [_rand_level(rng, 3, gh, gw, 3, 5, 3, np.float32) * np.float32(0.7) for gh, gw in ((2, 3), (4, 6))]   # products < 0.49
    return _case(lv, 5, 3, empty={0, 1, 2}, degenerate=True)


def _long_segments():
    """class 1 of image 0 holds 1 100 rows (18 mask tiles a side, past the 1 024 lanes of the walk), class 1 of image 1 holds
    100 (two tiles), class 1 of image 2 holds 40 other boxes; boxes spread over the image with sides in [0.2, 0.6): hard NMS
    suppresses most of every segment. Mixing rows of different images would show in all three."""
    rng = np.random.default_rng(14)
    B, g, A, C = 3, 22, 3, 3
    t = np.zeros((B, g * g * A, 5 + C), dtype=np.float32)
    plan = {0: ((1, 1100), (0, 150)), 1: ((1, 100), (2, 70)), 2: ((1, 40), (0, 30))}
    for b, segs in plan.items():
        slots = rng.permutation(g * g * A)
        at = 0
        for c, m in segs:
            s = slots[at:at + m]
            at += m
            t[b, s, 0:2] = rng.random((m, 2))
            t[b, s, 2:4] = 0.2 + 0.4 * rng.random((m, 2))
            t[b, s, 4] = 0.8 + 0.2 * rng.random(m)
            t[b, s, 5 + c] = 0.7 + 0.3 * rng.random(m)      # product >= 0.56; the other classes' products are 0
    return _case([t.reshape(B, g, g, A * (5 + C))], C, 3)


def _ties():
    """images 0 and 1 hold identical rows (equal scores that are never compared), and two boxes of each share conf and every
    class probability: exact ties inside the segments of the classes they pass in"""
    rng = np.random.default_rng(16)
    t = _rand_level(rng, 3, 4, 6, 3, 5, 3, np.float32).reshape(3, 4, 6, 3, 10)
    t[0, 0, 0, 0, 4:] = t[0, 2, 3, 1, 4:]
    t[0, 0, 0, 0, 4] = t[0, 2, 3, 1, 4] = np.float32(0.95)
    t[0, 0, 0, 0, 5 + 2] = t[0, 2, 3, 1, 5 + 2] = np.float32(0.9)
    t[1] = t[0]
    return _case([t.reshape(3, 4, 6, 30)], 5, 3, ties=True)


def _simple(seed, B, grids, A, C, version):
    rng = np.random.default_rng(seed)
    return _case([_rand_level(rng, B, gh, gw, A, C, version, np.float32) for gh, gw in grids], C, version)


BUILDERS = {
    "boundaries-f32": lambda: _boundaries(np.float32),
    "boundaries-f64": lambda: _boundaries(np.float64),
    "empty-middle": _empty_middle,
    "all-empty": _all_empty,
    "v1-layout": lambda: _simple(21, 3, ((5, 7),), 2, 5, 1),          # D = 5 A + C
    "v2-layout": lambda: _simple(22, 3, ((5, 7),), 5, 4, 2),
    "one-class": lambda: _simple(23, 3, ((6, 8),), 3, 1, 3),
    "long-segments": _long_segments,
    "2160-segments": lambda: _simple(24, 27, ((2, 2),), 3, 80, 3),     # past NMS_LDS_CLASSES = 2 048
    "ties": _ties,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ---- expected values: the oracle, per image (computed once per case and mode) ----------------------------------------
def _oracle_nms(rows, C, mode):
    if mode == 0 or rows.shape[0] == 0:
        return rows
    if mode == 1:
        return OT.nms(rows, C, NMS_THR)
    if mode == 2:
        return OT.soft_nms(rows, C, NMS_THR, THR, SIGMA)
    return OT.nms(rows, C, NMS_THR, 2)


@functools.lru_cache(maxsize=None)
def oracle_decoded(name):
    c = case(name)
    B = c["levels"][0].shape[0]
    return [np.asarray(OT.decode(*[lv[b] for lv in c["levels"]], class_num=c["C"], threshold=THR,
                                 version=c["version"])).reshape(-1, 7) for b in range(B)]


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    return [np.asarray(_oracle_nms(r, case(name)["C"], mode)).reshape(-1, 7) for r in oracle_decoded(name)]


def check_not_vacuous(name, mode):
    """the conditions of the module docstring, on the oracle's output alone"""
    c = case(name)
    dec, exp = oracle_decoded(name), expected(name, mode)
    for b, rows in enumerate(dec):
        assert (rows.shape[0] == 0) == (b in c["empty"]), (name, b, rows.shape)
        if not c["ties"]:      # the oracle is only a reference where it has no exact tie to order
            for k in range(c["C"]):
                s = (rows[:, 4] * rows[:, 6])[rows[:, 5].astype(int) == k]
                assert len(np.unique(s)) == len(s), (name, b, k)
    if c["degenerate"]:
        assert all(e.shape == (0, 7) for e in exp)
        return
    assert sum(e.shape[0] > 0 for e in exp) >= 2, name
    if mode != 0:
        hard = expected(name, 1)
        assert sum(h.shape[0] < d.shape[0] for h, d in zip(hard, dec)) >= 2, name


# ---- the device ----------------------------------------------------------------------------------------------------
def _detect(name, mode, **kw):
    from tf2_yolo_amd import tools
    c = case(name)
    return tools.detect_batch(*c["levels"], class_num=c["C"], conf_threshold=THR, nms_mode=mode, nms_threshold=NMS_THR,
                              nms_sigma=SIGMA, version=c["version"], **kw)


def _per_image_device(name, mode):
    from tf2_yolo_amd import tools
    c = case(name)
    C, out = c["C"], []
    for b in range(c["levels"][0].shape[0]):
        rows = tools.decode(*[lv[b] for lv in c["levels"]], class_num=C, threshold=THR, version=c["version"])
        if mode and rows.size:
            rows = (tools.nms(rows, C, NMS_THR) if mode == 1 else
                    tools.soft_nms(rows, C, NMS_THR, THR, SIGMA) if mode == 2 else tools.nms(rows, C, NMS_THR, 2))
        out.append(np.asarray(rows).reshape(-1, 7))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == w.shape, (what, b, g.shape, w.shape)
        assert np.array_equal(g, w), (what, b)


def _check(name, mode, oracle=True):
    check_not_vacuous(name, mode)
    got = _detect(name, mode)
    if oracle:
        _same(got, expected(name, mode), f"{name} mode {mode} vs oracle")
    _same(got, _per_image_device(name, mode), f"{name} mode {mode} vs per-image device path")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["boundaries-f32", "boundaries-f64"])
def test_image_boundaries_inside_decode_blocks(name, mode):
    _check(name, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_empty_images(mode):
    _check("empty-middle", mode)
    exp = expected("empty-middle", mode)
    assert exp[1].shape == (0, 7) and set(exp[2][:, 5]) == {3.0}


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_without_any_candidate(mode):
    _check("all-empty", mode)
    assert [g.shape for g in _detect("all-empty", mode)] == [(0, 7)] * 3


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["v1-layout", "v2-layout", "one-class"])
def test_other_layouts(name, mode):
    _check(name, mode)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_segments_past_a_mask_tile_and_past_the_walk(mode):
    dec = oracle_decoded("long-segments")
    assert (dec[0][:, 5] == 1).sum() > 1024 and (dec[1][:, 5] == 1).sum() > 64 and (dec[2][:, 5] == 1).sum() > 0
    _check("long-segments", mode)


def test_long_segments_on_the_walk_kernels():
    """yolo_set_option(YOLO_OPT_NMS_WALK): no bit matrices, every segment on the walk / tiled kernels -- the path the batched
    call also takes when its matrix buffer is too small"""
    from tf2_yolo_amd import ops
    check_not_vacuous("long-segments", 1)
    try:
        ops.set_option(7, 1)
        for mode in (1, 2):
            _same(_detect("long-segments", mode), expected("long-segments", mode), f"walk kernels, mode {mode}")
    finally:
        ops.reset_options()


@pytest.mark.parametrize("mode", [1, 2])
def test_call_without_a_matrix_buffer(mode):
    """the C entry points with mask = NULL although the segment scan asks for words: nms_mask_fit_kernel takes every segment
    off the bit matrices, the walk / tiled kernels give the same rows"""
    from tf2_yolo_amd import _lib, ops
    c = case("long-segments")
    check_not_vacuous("long-segments", mode)
    rows, img_off = ops.decode_batch([torch.from_numpy(lv).cuda() for lv in c["levels"]], [3], c["C"], 3, [THR])
    n, B, lib = int(rows.shape[0]), 3, _lib.load()
    nbytes = int(lib.yolo_nms_batch_workspace_bytes(n, B, c["C"]))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    words = torch.zeros(1, device="cuda", dtype=torch.int64)
    _lib.check(lib.yolo_nms_batch_prepare(ops._p(rows), n, ops._p(img_off), B, c["C"], ops._p(words), ops._p(ws), nbytes,
                                          ops._stream()), "yolo_nms_batch_prepare")
    assert int(words.item()) >= 1100 * 18          # the 1 100-row segment alone: 18 words a row
    keep = torch.empty(n, device="cuda", dtype=torch.uint8)
    out = torch.empty((n, 7), device="cuda", dtype=torch.float64)
    kept_off = torch.empty(B + 1, device="cuda", dtype=torch.int32)
    _lib.check(lib.yolo_nms_batch_select(ops._p(rows), n, B, c["C"], {1: _lib.NMS_HARD, 2: _lib.NMS_SOFT}[mode], NMS_THR, THR,
                                         SIGMA, None, 0, ops._p(keep), ops._p(out), ops._p(kept_off), ops._p(ws), nbytes,
                                         ops._stream()), "yolo_nms_batch_select")
    offs = kept_off.cpu().numpy()
    assert offs[0] == 0 and np.all(np.diff(offs) >= 0)
    _same([out[int(offs[b]):int(offs[b + 1])].cpu().numpy() for b in range(B)], expected("long-segments", mode),
          f"no matrix buffer, mode {mode}")


@pytest.mark.parametrize("mode", [1, 2])
def test_more_segments_than_the_lds_tables_hold(mode):
    c = case("2160-segments")
    assert c["levels"][0].shape[0] * c["C"] == 2160
    _check("2160-segments", mode)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_tie_order(mode):
    dec = oracle_decoded("ties")
    assert np.array_equal(dec[0], dec[1])
    s = (dec[0][:, 4] * dec[0][:, 6])[dec[0][:, 5] == 2]
    assert len(np.unique(s)) < len(s)                      # an exact tie inside one segment
    _check("ties", mode, oracle=False)
    got = _detect("ties", mode)
    assert np.array_equal(got[0], got[1])


def test_cuda_tensors_in_cuda_tensors_out():
    from tf2_yolo_amd import tools
    c = case("boundaries-f32")
    check_not_vacuous("boundaries-f32", 1)
    levels = [torch.from_numpy(lv).cuda() for lv in c["levels"]]
    before = [lv.clone() for lv in levels]
    got = tools.detect_batch(*levels, class_num=c["C"], conf_threshold=THR, nms_mode=1, nms_threshold=NMS_THR, version=3)
    assert all(torch.is_tensor(g) and g.is_cuda and g.dtype == torch.float64 for g in got)
    _same([g.cpu().numpy() for g in got], expected("boundaries-f32", 1), "CUDA tensors")
    assert all(torch.equal(a, b) for a, b in zip(levels, before))       # used in place, left alone


# ---- Model.detect ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tiny-v3-64", "v2-64"])
def net_case(request):
    import gc
    from test_gpu_predict_fp16 import _setup
    kw = dict(version=3, hw=64, N=5, tiny=True) if request.param == "tiny-v3-64" else dict(version=2, hw=64, N=5)
    y, model, fwd, x = _setup(**kw)
    assert len(x) == 5
    yield model, x
    del y, model
    gc.collect()
    torch.cuda.empty_cache()


def _listed(p):
    return p if isinstance(p, list) else [p]


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_detect(net_case, precision):
    """len(x) = 5 with batch_size = 2: three chunks, the last one short. Equal to tools._detections per image of predict's
    arrays; detect twice with a predict in between gives the same arrays."""
    from tf2_yolo_amd import tools
    model, x = net_case
    C = next(u.C for u in model.net.units if u.kind == "head")
    pred = _listed(model.predict(x, batch_size=2, precision=precision))
    # a threshold low enough that rows exist: the 300th largest conf * prob product of the batch
    prods = []
    for lv in pred:
        A = lv.shape[-1] // (5 + C)
        t = lv.reshape(*lv.shape[:3], A, 5 + C)
        prods.append((t[..., 4:5] * t[..., 5:]).ravel())
    prods = np.concatenate(prods)
    thr = float(np.sort(prods)[-300])
    for mode in (1, 2):
        want = [tools._detections([lv[b] for lv in pred], C, thr, mode, NMS_THR, SIGMA, model.version) for b in range(5)]
        assert sum(w.shape[0] for w in want) > 0 and sum(w.shape[0] > 0 for w in want) >= 2
        kw = dict(batch_size=2, precision=precision, conf_threshold=thr, nms_mode=mode, nms_threshold=NMS_THR, nms_sigma=SIGMA)
        got = model.detect(x, **kw)
        _same(got, want, f"Model.detect {precision} mode {mode}")
        again = _listed(model.predict(x, batch_size=2, precision=precision))
        assert all(np.array_equal(a, b) for a, b in zip(pred, again))
        _same(model.detect(x, **kw), got, "Model.detect, second call")


def test_model_detect_refuses_a_classifier_and_bad_modes(net_case):
    model, x = net_case
    with pytest.raises(ValueError, match="nms_mode"):
        model.detect(x, nms_mode=4)
    with pytest.raises(ValueError, match="precision"):
        model.detect(x, precision="int8")
    version, model.version = model.version, 0
    try:
        with pytest.raises(ValueError, match="classifier"):
            model.detect(x)
    finally:
        model.version = version
