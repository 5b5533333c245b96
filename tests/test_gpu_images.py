"""Raw uint8 images in (tf2_yolo_amd/images.py, csrc/image.hip): the kernel against the float64 oracle of
tests/image_cases.py, the exact cases bit for bit, and the rescale= / resize= keywords of predict, detect_images, fit and evaluate
against the same calls on host-converted float32 arrays.

The bar of the resampled cases is |out - oracle| <= 4e-4 |rescale| grey levels: at most about 12 float32 roundings on
magnitudes <= 255 (four uint8 -> float conversions are exact; two fractions, three differences, three products and three sums
of the two lerps, one rescale) are <= 12 * 255 * 2^-24 = 1.8e-4, and the bar is twice that. A wrong tap or a half-pixel slip
costs >= 0.1 grey levels on random images."""
import numpy as np
import pytest
import torch

import image_cases as IC

pytestmark = pytest.mark.gpu

S = 1 / 255
LOSS_RTOL = 1e-12      # reported float64 losses of two runs on EQUAL weights and inputs (test_fit_on_uint8_...: the derivation)
A9 = [[0.89663461, 0.78365384], [0.375, 0.47596153], [0.27884615, 0.21634615], [0.14182692, 0.28605769],
      [0.14903846, 0.10817307], [0.07211538, 0.14663461], [0.07932692, 0.05528846], [0.03846153, 0.07211538],
      [0.02403846, 0.03125]]


def _host_f32(x, s):
    return x.astype(np.float32) * np.float32(1.0 if s is None else s)


# ---- the kernel ------------------------------------------------------------------------------------------------------
# (9, 7): W * 3 = 21 is no multiple of 4 -- the scalar-store form of the kernel
@pytest.mark.parametrize("rescale", IC.RESCALES, ids=["div255", "none"])
@pytest.mark.parametrize("resize", ["stretch", "letterbox"])
@pytest.mark.parametrize("out_hw", IC.OUTPUT_SIZES + [(9, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_the_oracle(out_hw, resize, rescale):
    """every source size in ONE call (byte offsets 3, 30, 1830, 1935, 3618, 41739: odd and unaligned)"""
    from tf2_yolo_amd import images
    imgs = IC.source_images()
    x, geom = images.prepare(imgs, out_hw, rescale=rescale, resize=resize, pad_grey=IC.PAD_GREY)
    assert x.dtype == torch.float32 and x.is_cuda and tuple(x.shape) == (len(imgs), *out_hw, 3)
    assert isinstance(geom, np.ndarray) and geom.dtype == np.int32 and geom.shape == (len(imgs), 4)
    geo = images.letterbox_geometry if resize == "letterbox" else images.stretch_geometry
    assert [tuple(g) for g in geom] == [geo(s, out_hw) for s in IC.SOURCE_SIZES]
    want, is_pad = IC.oracle_prepare(imgs, out_hw, geom, rescale)
    got = x.cpu().numpy()
    s = 1.0 if rescale is None else rescale
    err = np.abs(got.astype(np.float64) - want)
    worst = [float(err[i][~is_pad[i]].max()) / s for i in range(len(imgs))]
    print(f"{out_hw} {resize} rescale {rescale}: worst |out - oracle| per image, grey levels: " + " ".join(f"{w:.2e}" for w in worst))
    assert max(worst) <= 4e-4
    assert is_pad.any() == (resize == "letterbox")
    assert np.array_equal(got[is_pad], want[is_pad].astype(np.float32))        # padding: bit-exact
    again, _ = images.prepare(imgs, out_hw, rescale=rescale, resize=resize, pad_grey=IC.PAD_GREY, out=torch.empty_like(x))
    assert torch.equal(again, x)


@pytest.mark.parametrize("rescale", IC.RESCALES, ids=["div255", "none"])
def test_equal_size_is_bit_identical_to_the_host_conversion(rescale):
    from tf2_yolo_amd import images
    x = np.random.default_rng(1).integers(0, 256, (3, 64, 32, 3), dtype=np.uint8)
    x[0, 0, 0], x[0, 0, 1] = 0, 255
    want = _host_f32(x, rescale)
    for resize in (None, "stretch", "letterbox"):
        got, geom = images.prepare(x, (64, 32), rescale=rescale, resize=resize)
        assert np.array_equal(got.cpu().numpy(), want), f"ndarray, resize {resize}"
        assert [tuple(g) for g in geom] == [(0, 0, 64, 32)] * 3
    xd = torch.from_numpy(x).cuda()
    got, _ = images.prepare(xd, (64, 32), rescale=rescale, resize=None)
    assert np.array_equal(got.cpu().numpy(), want), "CUDA tensor"
    got, _ = images.prepare(xd[:2], (64, 32), rescale=rescale, resize=None)      # a shorter batch on the cached table
    assert np.array_equal(got.cpu().numpy(), want[:2])
    got, _ = images.prepare([a for a in x], (64, 32), rescale=rescale, resize=None)
    assert np.array_equal(got.cpu().numpy(), want), "list of images"
    # a CUDA tensor resized: the same taps as the host path
    a, _ = images.prepare(xd, (32, 64), rescale=rescale, resize="letterbox")
    b, _ = images.prepare(x, (32, 64), rescale=rescale, resize="letterbox")
    assert torch.equal(a, b)


def test_past_the_grid_cap():
    """1 208 064 float4 work items = 2.3 stream caps (tests/test_images_cpu.py asserts the band): some threads run a first, a
    middle and a last pass"""
    from tf2_yolo_amd import images
    h, w = IC.PAST_CAP_HW
    x = np.random.default_rng(2).integers(0, 256, (IC.PAST_CAP_N, h, w, 3), dtype=np.uint8)
    got, _ = images.prepare(x, (h, w), rescale=S, resize=None)
    assert np.array_equal(got.cpu().numpy(), _host_f32(x, S))


def test_bad_table_entries_come_out_all_pad():
    """The kernel checks every entry against the byte count it is given and never dereferences one whose extent leaves the
    buffer (or whose sizes are not positive): that image is all pad, its neighbours are untouched."""
    from tf2_yolo_amd import images, ops
    imgs = IC.source_images()
    out_hw = (32, 64)
    p = images.plan(imgs, out_hw, rescale=S, resize="letterbox")
    good, _ = images.prepare(imgs, out_hw, rescale=S, resize="letterbox")
    good = good.cpu().numpy()
    src = torch.from_numpy(np.concatenate([a.ravel() for a in imgs])).cuda()
    assert src.numel() == p.src_bytes
    table = p.table.copy()
    table["off"][2] = p.src_bytes - 10          # 1800 bytes from there leave the buffer
    table["sh"][4] = 0                          # no rows
    table["off"][5] = -1                        # in front of the buffer
    table["off"][6] += 1                        # the last image, one byte too far
    bad = {2, 4, 5, 6}
    out = torch.full((len(imgs), *out_hw, 3), -1.0, device="cuda")
    ops.image_prepare(src, p.src_bytes, torch.from_numpy(table.view(np.uint8).copy()).cuda(), len(imgs), out, S, IC.PAD_GREY)
    got = out.cpu().numpy()
    pad = np.float32(IC.PAD_GREY) * np.float32(S)
    for i in range(len(imgs)):
        assert np.array_equal(got[i], np.full_like(got[i], pad) if i in bad else good[i]), i


def test_library_refuses_bad_sizes():
    from tf2_yolo_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16, device="cuda")
    p, o = buf.data_ptr(), out.data_ptr()
    for args in ((None, 64, p, 1, 1, 1), (p, 64, None, 1, 1, 1), (p, 0, p, 1, 1, 1), (p, 64, p, 0, 1, 1), (p, 64, p, 1, 0, 1),
                 (p, 64, p, 1, 1, -1), (p, 64, p, 1, 4097, 1), (p, 64, p, 1, 1, 4097)):
        assert lib.yolo_image_prepare(*args, 1.0, 128.0, o, None) == -1, args
    assert lib.yolo_image_prepare(p, 64, p, 1, 1, 1, 1.0, 128.0, None, None) == -1
    torch.cuda.synchronize()


# ---- predict / detect --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    import gc
    from test_gpu_predict_fp16 import _setup
    y, model, fwd, x = _setup(version=3, hw=64, N=5, tiny=True)
    model.facade = y
    yield model
    del y, model
    gc.collect()
    torch.cuda.empty_cache()


def _listed(p):
    return p if isinstance(p, list) else [p]


def _same_arrays(a, b):
    a, b = _listed(a), _listed(b)
    return len(a) == len(b) and all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(a, b))


def test_predict_uint8_equals_predict_of_the_host_conversion(detector):
    """5 images in chunks of 2: three chunks, the last one short"""
    x = np.random.default_rng(4).integers(0, 256, (5, 64, 64, 3), dtype=np.uint8)
    want = detector.predict(_host_f32(x, S), batch_size=2)
    assert _same_arrays(detector.predict(x, batch_size=2, rescale=S), want)
    assert _same_arrays(detector.predict(torch.from_numpy(x).cuda(), batch_size=2, rescale=S), want)
    assert not _same_arrays(detector.predict(x, batch_size=2), want)           # without the keyword: the pixels as they are
    assert _same_arrays(detector.predict(x, batch_size=2, resize="stretch"), detector.predict(x.astype(np.float32), batch_size=2))
    with pytest.raises(ValueError, match="network input"):
        detector.predict(x[:, :32], rescale=S)
    with pytest.raises(TypeError):
        detector.predict(_host_f32(x, S), rescale=S)
    with pytest.raises(ValueError, match="resize"):
        detector.predict(x, resize="bicubic")


def test_predict_and_detect_on_a_list_of_mixed_sizes(detector):
    from tf2_yolo_amd import images
    imgs = IC.source_images()            # 7 images in chunks of 3: 3 + 3 + 1
    hw = (64, 64)
    prepared, geom = images.prepare(imgs, hw, rescale=S, resize="stretch")
    assert _same_arrays(detector.predict(imgs, batch_size=3, rescale=S, resize="stretch"), detector.predict(prepared, batch_size=3))
    boxed, geom = images.prepare(imgs, hw, rescale=S, resize="letterbox")
    pred = _listed(detector.predict(boxed, batch_size=3))
    assert _same_arrays(detector.predict(tuple(imgs), batch_size=3, rescale=S, resize="letterbox"), pred)
    C = next(u.C for u in detector.net.units if u.kind == "head")
    prods = []
    for lv in pred:
        t = lv.reshape(*lv.shape[:3], lv.shape[-1] // (5 + C), 5 + C)
        prods.append((t[..., 4:5] * t[..., 5:]).ravel())
    thr = float(np.sort(np.concatenate(prods))[-300])
    plain = detector.detect(boxed, batch_size=3, conf_threshold=thr)
    got = detector.detect_images(imgs, batch_size=3, conf_threshold=thr, rescale=S, resize="letterbox")
    assert isinstance(got, list) and len(got) == len(imgs) == len(plain)
    assert sum(r.shape[0] for r in plain) > 0 and sum(r.shape[0] > 0 for r in plain) >= 2
    moved = 0
    for r, q, g in zip(got, plain, geom):
        assert r.dtype == np.float64 and r.shape == q.shape
        assert np.array_equal(r, images.unletterbox(q, g, hw))
        moved += int(r.shape[0] > 0 and not np.array_equal(r, q))
    assert moved >= 1                                                          # some image's boxes were mapped back
    stretched = detector.detect_images(imgs, batch_size=3, conf_threshold=thr, rescale=S, resize="stretch")
    assert _same_arrays(stretched, detector.detect(prepared, batch_size=3, conf_threshold=thr))


def test_evaluate_on_uint8_equals_the_float_run(detector):
    """on the detector of the predict tests (moving statistics that keep an inference pass finite); 5 images in batches of 2"""
    import test_gpu_model as T
    from tf2_yolo_amd.optimizers import SGD
    y = detector.facade
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (5, 64, 64, 3), dtype=np.uint8)
    ys = [T._labels(rng, 5, g, y.class_num) for g in ((2, 2), (4, 4))]
    detector.compile(optimizer=SGD(learning_rate=0.0), loss=y.loss())
    want = detector.evaluate(_host_f32(x, S), ys, batch_size=2, verbose=0)
    got = detector.evaluate(x, ys, batch_size=2, verbose=0, rescale=S)
    print("evaluate", want, got)
    assert np.isfinite(want).all() and np.all(np.asarray(want) > 0)
    np.testing.assert_allclose(got, want, rtol=LOSS_RTOL, atol=0)
    assert not np.allclose(detector.evaluate(x, ys, batch_size=2, verbose=0), want, rtol=1e-3)     # without the keyword: 0 .. 255
    one = detector.test_on_batch(_host_f32(x[:2], S), [a[:2] for a in ys])
    assert np.isfinite(one).all()
    np.testing.assert_allclose(detector.test_on_batch(x[:2], [a[:2] for a in ys], rescale=S), one, rtol=LOSS_RTOL, atol=0)


# ---- fit / evaluate ----------------------------------------------------------------------------------------------------
class _Seq:
    def __init__(self, x, ys, bs):
        self.x, self.ys, self.bs = x, ys, bs

    def __len__(self):
        return len(self.x) // self.bs

    def __getitem__(self, i):
        sl = slice(i * self.bs, (i + 1) * self.bs)
        return self.x[sl], [y[sl] for y in self.ys]


@pytest.fixture(scope="module")
def train_data():
    from tf2_yolo_amd import labels
    rng = np.random.default_rng(3)
    _, ys = labels.synthetic_batch(rng, 26, (96, 96), 8)
    return rng.integers(0, 256, (26, 96, 96, 3), dtype=np.uint8), ys


def _trained(x, ys, **kw):
    import yolov3
    from tf2_yolo_amd.optimizers import Adam
    y = yolov3.Yolo((96, 96, 3), list("abcdefgh"))
    y.create_model(anchors=A9, pretrained_body=None, seed=11)
    m = y.model
    m.compile(optimizer=Adam(learning_rate=1e-3), loss=y.loss())
    start = m.net.params.data.clone()
    h = m.fit(x, ys, batch_size=4, epochs=2, verbose=0, shuffle=False, **kw)
    h2 = m.fit(_Seq(x, ys, 5), epochs=1, verbose=0, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(start, m.net.params.data)
    return m, h.history["loss"] + h2.history["loss"]


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_fit_on_uint8_is_bit_identical_to_fit_on_the_host_conversion(train_data, pipeline, monkeypatch):
    """26 images in batches of 4: 7 batches per epoch, the last one of 2 -- more batches than staging slots (3) or device sets
    (2); then a Sequence source of uint8 batches. Same seed, same order: weights, moving statistics and Adam moments must be
    EQUAL, since training is bit-reproducible and the device conversion is exact -- anything else is an ordering or conversion
    bug. The REPORTED losses (history; evaluate in test_evaluate_on_uint8_equals_the_float_run) are float64 sums that the loss kernel gathers with atomics in whatever order
    the waves finish: two runs of the float32 arm alone differ in their last bits (measured: 359.6481201650399 against
    359.64812016503987 with bit-equal weights, in the pipelined and in the plain loop alike), so they are compared to
    LOSS_RTOL = 1e-12: a sum of at most ~8 000 float64 terms (cells x anchors of a batch) in another order moves by at most
    8 000 x 2^-53 = 9e-13 of the sum of magnitudes."""
    monkeypatch.setenv("YOLO_FIT_PIPELINE", pipeline)
    x, ys = train_data
    a, hist_a = _trained(_host_f32(x, S), ys)
    b, hist_b = _trained(x, ys, rescale=S)
    assert np.isfinite(hist_a).all() and len(hist_a) == len(hist_b) == 3
    print("history", hist_a, hist_b)
    np.testing.assert_allclose(hist_b, hist_a, rtol=LOSS_RTOL, atol=0)
    for p, q in ((a.net.params.data, b.net.params.data), (a.net.state.data, b.net.state.data),
                 (a.optimizer.m, b.optimizer.m), (a.optimizer.v, b.optimizer.v)):
        assert torch.equal(p, q)
    if pipeline == "1":
        assert b._feed_bufs.dev_sets[0][0].dtype == torch.uint8 and b._feed_bufs.dev_x32[0].dtype == torch.float32
        assert b._feed_bufs.slots[0].bufs[0].dtype == torch.uint8 and b._feed_bufs.slots[0].bufs[1].dtype == torch.float32
        assert a._feed_bufs.dev_sets[0][0].dtype == torch.float32 and a._feed_bufs.dev_x32[0] is None


def test_training_calls_refuse_what_they_cannot_rescale(train_data):
    import yolov3
    from tf2_yolo_amd.optimizers import SGD
    x, ys = train_data
    y = yolov3.Yolo((96, 96, 3), list("abcdefgh"))
    y.create_model(anchors=A9, pretrained_body=None, seed=11)
    m = y.model
    m.compile(optimizer=SGD(learning_rate=1e-4), loss=y.loss())
    with pytest.raises(TypeError, match="uint8"):
        m.fit(_host_f32(x, S), ys, batch_size=4, verbose=0, rescale=S)
    with pytest.raises(ValueError, match="does not resize"):
        m.fit(x[:, :64, :64], ys, batch_size=4, verbose=0, rescale=S)
    with pytest.raises(ValueError, match="network input"):
        m.train_on_batch(x[:4, :64], [a[:4] for a in ys], rescale=S)
    with pytest.raises(TypeError, match="uint8"):
        m.test_on_batch(_host_f32(x[:4], S), [a[:4] for a in ys], rescale=S)
    r = m.train_on_batch(x[:4], [a[:4] for a in ys], rescale=S)
    assert np.isfinite(r).all()
