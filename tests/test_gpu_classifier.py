"""The backbone classifiers (bodies.darknet / darknet19 / darknet53 / csp_darknet53) on the device. The Dense-topped three:
the top against tests/classifier_ref.py from the trunk's own feature map, the hand-over to a detector, reproducibility, the
recorded step, data-parallel bookkeeping, half-precision predict and the weights round trip. darknet19: the whole graph
against a float64 oracle (tests/classifier_oracle.py), every parameter gradient; recorded against eager steps; and that it
learns. Inputs are 64 x 64 unless a case says otherwise. Bar: 1e-4 of the largest entry of the compared tensor, the
project's fp32 bar; gradient tensors of the full-parity test 1e-3 in relative L2."""
import gc

import numpy as np
import pytest
import torch

import classifier_ref as R
import test_gpu_model as T

pytestmark = pytest.mark.gpu

TOL = 1e-4
K = 5

# id -> (constructor, input shape, feature map (h, w), detector's (yolo_body, yolo_head, head arguments))
CASES = {
    "darknet53": ("darknet53", (64, 64, 3), (2, 2)),
    "csp_darknet53": ("csp_darknet53", (64, 64, 3), (2, 2)),
    "darknet": ("darknet", (128, 128, 3), (2, 2)),
    "darknet53-96x160": ("darknet53", (96, 160, 3), (3, 5)),
}


def _ctor(name):
    from tf2_yolo_amd import bodies
    return getattr(bodies, name)


def _make(name, shape, include_top=True, class_num=K):
    if name == "darknet":
        assert include_top
        return _ctor(name)(input_shape=shape, class_num=class_num)
    return _ctor(name)(include_top=include_top, weights=None, input_shape=shape, class_num=class_num)


def _trunk_of(name, shape):
    """the trunk alone: include_top=False where the constructor has it; v1.5's darknet() has no such argument, its trunk is
    the whole body of the detector"""
    if name != "darknet":
        return _make(name, shape, include_top=False)
    from tf2_yolo_amd import graphs
    from tf2_yolo_amd.model import Model
    return Model(graphs.build_darknet(shape, K, include_top=False), version=0)


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    name, shape, fmap = CASES[request.param]
    rng = np.random.default_rng(7)
    clf = _make(name, shape)
    T._perturb(clf, rng)       # non-trivial BatchNorm parameters, biases and moving statistics; he-scaled kernels
    N = 2
    x = rng.random((N,) + shape, dtype=np.float32)
    t = R.one_hot(rng.integers(0, K, N), K).astype(np.float32)
    c = {"id": request.param, "name": name, "shape": shape, "fmap": fmap, "clf": clf, "x": x, "t": t}
    yield c
    del c["clf"], clf
    _free()


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def _state(m):
    return m.net.params.data.clone(), m.net.state.data.clone()


def _restore(m, saved):
    m.net.before_param_write()
    m.net.params.data.copy_(saved[0])
    m.net.state.data.copy_(saved[1])
    m.net.mark_params_changed()


def test_structure(case):
    clf = case["clf"]
    assert clf.output_shape == (None, K) and clf.output.shape == (None, K)
    names = clf.layer_names()
    assert names[-2:] == ["top_gap", "top_dense"]
    kernel, bias = clf.get_layer("top_dense").get_weights()
    assert kernel.shape == (1024, K) and bias.shape == (K,)
    assert clf.get_layer("top_gap").get_weights() == []
    from tf2_yolo_amd import engine
    assert clf.count_params() == sum(engine.count_params(clf.net))
    p = clf.predict(case["x"])
    assert p.shape == (2, K) and np.abs(p.sum(axis=1) - 1).max() < 1e-5
    assert np.array_equal(clf(case["x"]).cpu().numpy(), p)


def test_top_against_the_reference_and_the_hand_over_to_a_detector(case):
    """Wiring and top: the include_top=False model, given the classifier's trunk weights through the public API, yields the
    feature map F in training mode; from F classifier_ref gives probabilities, loss and the gradients of top_dense."""
    from tf2_yolo_amd.losses import CategoricalCrossentropy
    clf, x, t, name, shape = case["clf"], case["x"], case["t"], case["name"], case["shape"]
    saved = _state(clf)
    trunk = _trunk_of(name, shape)
    trunk.set_body_weights(clf)
    F = trunk(x, training=True).cpu().numpy()
    assert F.shape == (2,) + case["fmap"] + (1024,)
    W, b = clf.get_layer("top_dense").get_weights()
    ref = R.top_from_features(F, W, b, t)

    net = clf.net
    net.grads.zero_()
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    p = net.forward(xd, training=True)[0]
    loss_buf, d = torch.zeros(8, device="cuda", dtype=torch.float64), torch.empty_like(p)
    CategoricalCrossentropy().fwd_bwd(td, p, grad_scale=1.0, dpred=d, loss_out=loss_buf)
    net.backward([d])
    torch.cuda.synchronize()
    u = net.units[-1]
    dW = net._gview(u.p_kernel).reshape(K, 1024).cpu().numpy().T
    db = net._gview(u.p_bias).cpu().numpy()
    errs = {"p": _rel(p.cpu().numpy(), ref["p"]), "loss": abs(float(loss_buf[0].item()) - ref["loss"]) / abs(ref["loss"]),
            "dW": _rel(dW, ref["dW"]), "db": _rel(db, ref["db"])}
    print(case["id"], errs)
    assert all(e <= TOL for e in errs.values()), errs
    assert np.abs(dW).max() > 0 and np.abs(net.grads.cpu().numpy()).max() > 0
    net.grads.zero_()       # (the optimizer step that would have cleared them did not run)
    # test_on_batch / evaluate: inference mode, the loss object and the metric by their compile strings
    clf.compile(optimizer="sgd", loss="categorical_crossentropy", metrics=["accuracy"])
    pi = clf.predict(x)
    lv, acc = clf.test_on_batch(x, t)
    assert abs(lv - R.cce(t, pi)) <= TOL * R.cce(t, pi) and acc == R.accuracy(t, pi)
    assert clf.evaluate(x, t, batch_size=2, verbose=0) == [lv, acc]
    _restore(clf, saved)

    # a detector takes the classifier as its pretrained backbone: every trunk layer equal, no layer of the top
    if name == "darknet":
        from yolov1_5.models import yolo_body, yolo_head
        det = yolo_head(yolo_body(shape, pretrained_darknet=clf), bbox_num=2, class_num=3)
    elif name == "darknet53":
        from yolov3.models import yolo_body, yolo_head
        det = yolo_head(yolo_body(shape, pretrained_darknet=clf), class_num=3)
    else:
        from yolov4.models import yolo_body, yolo_head
        det = yolo_head(yolo_body(shape, pretrained_darknet=clf), class_num=3)
    assert not [n for n in det.layer_names() if n.startswith("top_")]
    trunk_layers = trunk.layer_names()
    assert trunk_layers == clf.layer_names()[:-2] and len(trunk_layers) > 40
    for n in trunk_layers:
        for a, c in zip(det.get_layer(n).get_weights(), clf.get_layer(n).get_weights()):
            assert np.array_equal(a, c), n
    del det, trunk
    _free()


def _train(clf, x, t, steps, saved):
    from tf2_yolo_amd import optimizers
    _restore(clf, saved)
    clf.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss="categorical_crossentropy")
    x, t = torch.as_tensor(x).cuda(), torch.as_tensor(t).cuda()
    # (train_step_device: train_on_batch always asks for the metrics' values, and a step with metrics is never recorded)
    losses = [float(clf.train_step_device(x, [t])[0][0][0].item()) for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, clf.net.params.data.clone(), clf.net.state.data.clone()


@pytest.mark.parametrize("case", ["darknet53"], indirect=True)
def test_training_is_reproducible(case):
    clf, saved = case["clf"], _state(case["clf"])
    a, b = _train(clf, case["x"], case["t"], 3, saved), _train(clf, case["x"], case["t"], 3, saved)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[1], saved[0])
    u = clf.net.units[-1]
    s = u.p_kernel
    assert not torch.equal(a[1][s.offset:s.offset + s.size], saved[0][s.offset:s.offset + s.size])   # the top learns too
    _restore(clf, saved)


@pytest.mark.parametrize("case", ["darknet53", "csp_darknet53"], indirect=True)
def test_recorded_step_equals_the_eager_step(case, monkeypatch):
    clf, saved = case["clf"], _state(case["clf"])
    xd, td = torch.from_numpy(case["x"]).cuda(), torch.from_numpy(case["t"]).cuda()
    monkeypatch.delenv("YOLO_STEP_MODE", raising=False)
    monkeypatch.delenv("YOLO_STEP_GRAPH", raising=False)
    clf._graphs_failed = False
    rec = _train(clf, xd, td, 5, saved)
    assert clf._step_graphs is not None and not getattr(clf, "_graphs_failed", False)
    names = {name for _, _, name in clf._step_graphs.tape.entries}
    assert {"yolo_gap_fwd", "yolo_gap_bwd", "yolo_dense_softmax_fwd", "yolo_dense_softmax_bwd", "yolo_cce_fwd_bwd"} <= names
    monkeypatch.setenv("YOLO_STEP_MODE", "eager")
    eager = _train(clf, xd, td, 5, saved)
    assert clf._step_graphs is None
    assert rec[0] == eager[0] and torch.equal(rec[1], eager[1]) and torch.equal(rec[2], eager[2])
    _restore(clf, saved)


@pytest.mark.parametrize("case", ["darknet"], indirect=True)
def test_fit_with_the_compile_strings(case):
    from tf2_yolo_amd import optimizers
    clf, saved = case["clf"], _state(case["clf"])
    clf.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss="categorical_crossentropy", metrics=["acc"])
    h = clf.fit(case["x"], case["t"], batch_size=2, epochs=4, verbose=0, shuffle=False)
    assert len(h.history["loss"]) == 4 and all(np.isfinite(h.history["loss"]))
    r = clf.train_on_batch(case["x"], case["t"])
    assert len(r) == 2 and 0.0 <= r[1] <= 1.0
    with pytest.raises(ValueError, match="unknown loss"):
        clf.compile(loss="hinge")
    _restore(clf, saved)


def test_data_parallel_segments_cover_the_flat_buffer(case):
    from tf2_yolo_amd import dp
    net = case["clf"].net
    segs, units = dp.network_segments(net)
    assert units[0] is net.units[-1] and units[0].kind == "dense_softmax"
    cover = np.zeros(net.params.data.numel(), dtype=np.int32)
    for off, size in segs:
        cover[off:off + size] += 1
    assert (cover == 1).all()
    s = net.units[-1].p_kernel
    assert any(off <= s.offset and s.offset + s.size <= off + size for off, size in segs)
    # backward order: contiguous slices from the end of the buffer downwards
    assert segs[0][0] + segs[0][1] == net.params.data.numel()
    assert all(a[0] == b[0] + b[1] for a, b in zip(segs, segs[1:]))


def test_predict_fp16(case):
    """the trunk's planes convolutions on one fp16 pass, the top in fp32: rows still sum to 1; against the float64 oracle the
    bound of tests/test_gpu_predict_fp16.py (1.5 x the distance the fp16 rounding of the operands makes in the oracle itself).
    The oracle is oracle.models.yolov1_5_forward up to conv6_2 (its head gets zero weights and is not looked at) + classifier_ref."""
    clf, x = case["clf"], case["x"]
    p32, p16 = clf.predict(x), clf.predict(x, precision="fp16")
    assert p16.shape == (2, K) and np.abs(p16.sum(axis=1) - 1).max() < 1e-5 and np.isfinite(p16).all()
    assert np.array_equal(clf.predict(x), p32)
    if case["id"] != "darknet":
        return
    import test_gpu_predict_fp16 as H
    from oracle import models as OM
    w = T._weights_dict(clf)
    W, b = w.pop("top_dense/0"), w.pop("top_dense/1")
    w.update({"out1_xywhc_conv/0": np.zeros((1, 1, 1024, 10)), "out1_xywhc_conv/1": np.zeros(10),
              "out1_prob_conv/0": np.zeros((1, 1, 1024, 1)), "out1_prob_conv/1": np.zeros(1)})

    def fwd(w64, xt, training):
        _, c = OM.yolov1_5_forward(w64, xt, training=training)
        return [c.acts["conv6_2"]], c
    f64, fhalf = H._oracle(fwd, w, x, False)[0], H._oracle(fwd, w, x, True)[0]
    o64, ohalf = R.top_from_features(f64, W, b, case["t"])["p"], R.top_from_features(fhalf, W, b, case["t"])["p"]
    e_half, e_dev, e32 = _rel(ohalf, o64), _rel(p16, o64), _rel(p32, o64)
    print(f"fp16 predict: e_half {e_half:.3e} e_dev {e_dev:.3e} fp32 {e32:.3e}")
    assert e32 <= TOL
    assert e_dev <= 1.5 * e_half, (e_dev, e_half)


@pytest.mark.parametrize("case", ["darknet53", "darknet"], indirect=True)
def test_weights_round_trip(case, tmp_path):
    clf, x, name, shape = case["clf"], case["x"], case["name"], case["shape"]
    path = str(tmp_path / "clf.npz")
    clf.save_weights(path)
    fresh = _make(name, shape) if name == "darknet" else _ctor(name)(weights=path, input_shape=shape, class_num=K)
    if name == "darknet":
        assert not np.array_equal(fresh.predict(x), clf.predict(x))
        fresh.load_weights(path)
    assert np.array_equal(fresh.predict(x), clf.predict(x))
    del fresh
    if name == "darknet53":
        from yolov3.models import yolo_body, yolo_head
        det = yolo_head(yolo_body(shape), class_num=3)
        with pytest.raises(ValueError, match="missing"):
            det.load_weights(path)
        skipped = det.load_weights(path, by_name=True)
        assert skipped and all(not n.startswith(("conv1", "block")) for n in skipped)
        assert not [n for n in skipped if n.startswith("top_")]      # (the detector has no such layer to skip)
        for n in clf.layer_names()[:-2]:
            for a, c in zip(det.get_layer(n).get_weights(), clf.get_layer(n).get_weights()):
                assert np.array_equal(a, c), n
        del det
    _free()


# ---- darknet19: Conv2D_BN_Leaky(class_num, 1) + GlobalAveragePooling2D + Softmax ---------------------------------------------
def _darknet19(K, N, seed=11, perturb=True):
    from tf2_yolo_amd import bodies
    rng = np.random.default_rng(seed)
    clf = bodies.darknet19(input_shape=(64, 64, 3), class_num=K)
    if perturb:
        T._perturb(clf, rng)
    x = rng.random((N, 64, 64, 3), dtype=np.float32)
    t = R.one_hot(rng.integers(0, K, N), K).astype(np.float32)
    return clf, x, t


def test_darknet19_full_parity_against_the_float64_oracle():
    """N = 4, K = 3 (a BatchNormalization over three channels). The oracle (tests/classifier_oracle.py) takes the device's
    LeakyReLU branches and max-pool winners, as test_gpu_model.test_model_parity does; a forced decision may differ from the
    oracle's own only where |z| < 1e-4. Probabilities, loss and moving statistics at 1e-4 of the largest entry, every
    parameter gradient tensor within 1e-3 in the relative L2 norm."""
    import classifier_oracle as CO
    from tf2_yolo_amd.losses import CategoricalCrossentropy
    K, N = 3, 4
    clf, x, t = _darknet19(K, N)
    names = clf.layer_names()
    assert names[-4:] == ["top_conv", "top_bn", "top_gap", "top_softmax"] and clf.output_shape == (None, K)
    assert [a.shape for a in clf.get_layer("top_conv").get_weights()] == [(1, 1, 1024, K), (K,)]
    assert [a.shape for a in clf.get_layer("top_bn").get_weights()] == [(K,)] * 4
    w = T._weights_dict(clf)
    net = clf.net
    net.grads.zero_()
    p = net.forward(torch.from_numpy(x).cuda(), training=True)[0]
    masks = T._gpu_leaky_masks(net)
    loss_buf, d = torch.zeros(8, device="cuda", dtype=torch.float64), torch.empty_like(p)
    CategoricalCrossentropy().fwd_bwd(torch.from_numpy(t).cuda(), p, grad_scale=1.0, dpred=d, loss_out=loss_buf)
    net.backward([d])
    torch.cuda.synchronize()
    g = net.grads.cpu().numpy()

    wt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    p_ref, ctx = CO.darknet19_forward(wt, torch.tensor(x, dtype=torch.float64), True, True, masks)
    loss_ref = CO.cce(torch.tensor(t, dtype=torch.float64), p_ref)
    loss_ref.backward()
    assert "top" in ctx.mask_forced and len(ctx.pool_forced) == 5
    assert max(ctx.mask_disagree.values(), default=0.0) < 1e-4, ctx.mask_disagree
    assert max(ctx.pool_disagree.values(), default=0.0) < 1e-4, ctx.pool_disagree
    e_p = _rel(p.cpu().numpy(), p_ref.detach().numpy())
    e_l = abs(float(loss_buf[0].item()) - loss_ref.item()) / abs(loss_ref.item())
    print(f"darknet19 parity: probabilities {e_p:.3e} loss {e_l:.3e} forced leaky "
          f"{sum(a for a, _ in ctx.mask_forced.values())} pool {sum(a for a, _ in ctx.pool_forced.values())}")
    assert e_p <= TOL and e_l <= TOL
    for bn_name, (mm, mv) in ctx.moving.items():
        got = clf.get_layer(bn_name).get_weights()
        assert _rel(got[2], mm.detach().numpy()) <= TOL and _rel(got[3], mv.detach().numpy()) <= TOL, bn_name
    gmax = max(float(v.grad.abs().max()) for v in wt.values() if v.grad is not None)
    worst = ("", 0.0)
    for n in names:
        for i in range(len(clf.get_layer(n).get_weights())):
            r = wt[f"{n}/{i}"].grad
            if r is None:
                continue                      # moving statistics
            got = T._grad_view(clf, n, i, g)
            if n.endswith("_conv") and i == 1:
                assert np.abs(got).max() < 1e-4 * gmax, n       # a bias in front of BatchNormalization: exactly 0
                continue
            e = T._l2(got, r.numpy())
            worst = max(worst, (f"{n}/{i}", e), key=lambda v: v[1])
            assert e <= 1e-3, (n, i, e)
    print("darknet19 parity: worst gradient tensor (relative L2)", worst)
    # inference: the moving statistics, the bias inside the convolution
    wi = {k: torch.tensor(v, dtype=torch.float64) for k, v in T._weights_dict(clf).items()}
    with torch.no_grad():
        pi_ref = CO.darknet19_forward(wi, torch.tensor(x, dtype=torch.float64), False)[0].numpy()
    pi = clf.predict(x)
    assert _rel(pi, pi_ref) <= TOL and np.abs(pi.sum(axis=1) - 1).max() < 1e-5
    p16 = clf.predict(x, precision="fp16")
    assert p16.shape == (N, K) and np.abs(p16.sum(axis=1) - 1).max() < 1e-5
    # the hand-over to YOLOv2's body
    from yolov2.models import yolo_body, yolo_head
    det = yolo_head(yolo_body((64, 64, 3), pretrained_backbone=clf), class_num=3)
    assert not [n for n in det.layer_names() if n.startswith("top_")]
    for n in names[:-4]:
        for a, c in zip(det.get_layer(n).get_weights(), clf.get_layer(n).get_weights()):
            assert np.array_equal(a, c), n
    del det, clf
    _free()


def test_darknet19_recorded_step_and_reproducibility(monkeypatch):
    clf, x, t = _darknet19(3, 4)
    saved = _state(clf)
    monkeypatch.delenv("YOLO_STEP_MODE", raising=False)
    monkeypatch.delenv("YOLO_STEP_GRAPH", raising=False)
    rec = _train(clf, x, t, 5, saved)
    assert clf._step_graphs is not None and not getattr(clf, "_graphs_failed", False)
    names = {name for _, _, name in clf._step_graphs.tape.entries}
    assert {"yolo_bn_act_any_fwd", "yolo_bn_act_any_bwd", "yolo_gap_fwd", "yolo_dense_softmax_fwd"} <= names
    rec2 = _train(clf, x, t, 5, saved)
    monkeypatch.setenv("YOLO_STEP_MODE", "eager")
    eager = _train(clf, x, t, 5, saved)
    for other in (rec2, eager):
        assert rec[0] == other[0] and torch.equal(rec[1], other[1]) and torch.equal(rec[2], other[2])
    del clf
    _free()


LEARN_STEPS = 177


def test_darknet19_learns():
    """darknet19, two classes, eight 64 x 64 images: four with pixels in [0, 0.3], four in [0.7, 1]; Adam(1e-3), the
    constructor's own initialisation (seed 1234). The float64 oracle's training of this very problem
    (classifier_oracle.train on the same images, labels and initial weights, run on the CPU beforehand) has its loss at a
    quarter of the first step's, 0.90862 / 4 = 0.22716, at step 177 (0.22708) -- LEARN_STEPS. Its curve, loss at step
    1, 2, 3, 5, 10, 25, 50, 100, 150, 177, 200, 260:
      0.90862 0.37072 0.30691 0.29725 0.29414 0.28713 0.27595 0.25519 0.23644 0.22708 0.21950 0.20127
    (a fast drop while the class convolution separates the two clusters, then a slow one: the probabilities are a softmax
    of BatchNorm outputs, which only the slowly growing gamma can spread). The device must be below HALF of its first
    step's loss at that count, with every training image classified correctly."""
    from tf2_yolo_amd import bodies, optimizers
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0.0, 0.3, (4, 64, 64, 3)), rng.uniform(0.7, 1.0, (4, 64, 64, 3))]).astype(np.float32)
    t = np.zeros((8, 2), dtype=np.float32)
    t[:4, 0], t[4:, 1] = 1, 1
    clf = bodies.darknet19(input_shape=(64, 64, 3), class_num=2)
    clf.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss="categorical_crossentropy", metrics=["accuracy"])
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    bufs = [clf.train_step_device(xd, [td])[0][0].clone() for _ in range(LEARN_STEPS - 1)]     # (recorded steps, no metrics)
    last, acc = clf.train_on_batch(x, t)                                                        # step LEARN_STEPS, with accuracy
    losses = [float(b[0].item()) for b in bufs] + [last]
    print("darknet19 learns: loss at step 1, 2, 3, 10, 50, 100, 177:", [round(losses[i - 1], 5) for i in (1, 2, 3, 10, 50, 100, 177)])
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert acc == 1.0
    del clf
    _free()
