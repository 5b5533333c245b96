"""The recorded training step (capture.py: the launch tape of tape.py, or hipGraphs) inside a real session: steps
interleaved with inference, training-mode looks at the outputs, evaluate / predict, a partial batch, weights written from
outside, a step with metrics -- and Model.fit with validation data, which is exactly such a session.

Reference of every scenario: the SAME sequence of calls on a second model from the same seed with the recording switched
off (every step through Python). Bar, as in test_gpu_keras_shell.py::test_captured_step_is_bit_identical_to_eager_steps:
every loss equal to 1e-12 * max(|loss|, 1) (an fp64 sum whose atomics may change order); parameters, BatchNorm moving
statistics and both Adam moments bit-identical (8 classes = 39 head channels: every filter gradient runs on the
atomics-free kernels); inference outputs produced on the way bit-identical, NaN-aware (an untrained net in inference mode
may overflow, as in Keras). Two different batches alternate after the recording, so that neither stale inputs nor stale
weights can cancel. Every scenario pins which steps were eager, which one recorded and which replayed: one that stayed
eager would prove nothing."""
import collections
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A9 = [[0.89663461, 0.78365384], [0.375, 0.47596153], [0.27884615, 0.21634615], [0.14182692, 0.28605769],
      [0.14903846, 0.10817307], [0.07211538, 0.14663461], [0.07932692, 0.05528846], [0.03846153, 0.07211538],
      [0.02403846, 0.03125]]
HW, CLASSES = 96, 8
E, R, P = "eager", "record", "replay"


def _make(recording=True):
    import yolov3
    from tf2_yolo_amd.optimizers import Adam
    y = yolov3.Yolo((HW, HW, 3), list("abcdefgh"))
    y.create_model(anchors=A9, pretrained_body=None, seed=11)
    y.model.compile(optimizer=Adam(learning_rate=1e-3), loss=y.loss())
    y.model._graphs_failed = not recording       # eager reference: the switch a failed recording would flip
    return y.model


@pytest.fixture(scope="module")
def data():
    """host arrays of 14 rows (the fit cases) and two device batches of 4 (b1, b2) cut from them; never modified"""
    from tf2_yolo_amd import labels
    x, ys = labels.synthetic_batch(np.random.default_rng(3), 14, (HW, HW), CLASSES)
    dev = lambda sl: (torch.from_numpy(x[sl]).cuda(), [torch.from_numpy(a[sl]).cuda() for a in ys])
    return {"x": x, "ys": ys, "b1": dev(slice(0, 4)), "b2": dev(slice(4, 8)), "small": dev(slice(8, 10))}


@pytest.fixture(scope="module")
def clean_names(data):
    """multiset of the call names on the tape of an undisturbed recording: T, T, T (records) on a fresh model"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("YOLO_STEP_MODE", "tape")
        m = _make()
        for _ in range(3):
            m.train_step_device(*data["b1"])
        torch.cuda.synchronize()
    return _names(m)


def _names(m):
    return collections.Counter(name for _, _, name in m._step_graphs.tape.entries)


def _step(m, batch, kinds, with_metrics=False):
    """one training step; appends what it was (eager / record / replay) to `kinds`, returns the per-output losses"""
    g0 = m._step_graphs
    bufs, _ = m.train_step_device(*batch, with_metrics=with_metrics)
    g1 = m._step_graphs
    kinds.append(E if with_metrics or g1 is None else P if g1 is g0 else R)
    return [float(b[0].item()) for b in bufs]


def _final(m):
    torch.cuda.synchronize()
    return [t.clone() for t in (m.net.params.data, m.net.state.data, m.optimizer.m, m.optimizer.v)]


def _close(a, b):
    return a == b or (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * max(abs(a), 1.0)


def _same(a, b):
    """bit equality of two tensors / arrays, NaN == NaN"""
    if torch.is_tensor(a):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _compare(ref, got):
    """ref / got: (losses per step, [params, state, m, v], inference outputs). Prints the figures, then asserts the bar."""
    flat = lambda ls: [[v for v in (l if isinstance(l, (list, tuple)) else [l])] for l in ls]
    la, lb = flat(ref[0]), flat(got[0])
    first = next((i + 1 for i, (a, b) in enumerate(zip(la, lb)) if not all(_close(u, v) for u, v in zip(a, b))), None)
    diffs = [float((a.double() - b.double()).abs().max()) for a, b in zip(ref[1], got[1])]
    outs_same = [_same(a, b) for a, b in zip(ref[2], got[2])]
    print(f"\n[recording vs eager] first step whose loss differs: {first}; max |diff| params {diffs[0]:.3e} state "
          f"{diffs[1]:.3e} adam m {diffs[2]:.3e} adam v {diffs[3]:.3e}; inference outputs equal: {outs_same}")
    assert len(la) == len(lb) and first is None, (first, la, lb)
    for name, a, b in zip(("params", "state", "adam m", "adam v"), ref[1], got[1]):
        assert torch.equal(a, b), name
    assert len(ref[2]) == len(got[2]) and all(outs_same)


def _run_both(scenario, expect_kinds):
    """scenario(m, kinds) -> (losses, inference outputs); runs it eagerly and with the recording, compares, and returns the
    recording model"""
    res = {}
    for recording in (False, True):
        m = _make(recording)
        kinds = []
        losses, outs = scenario(m, kinds)
        res[recording] = (losses, _final(m), outs)
        if recording:
            assert kinds == expect_kinds, kinds
            assert m._step_graphs is not None
        else:
            assert set(kinds) == {E} and m._step_graphs is None
    _compare(res[False], res[True])
    assert res[True][0][2] != res[True][0][3]       # (b2 really went through the recording)
    return m


@pytest.mark.parametrize("mode", ["tape", "graph"])
def test_inference_before_the_recording(mode, monkeypatch, data, clean_names):
    """T, T, forward(training=False), T (records), T, T, T. The inference pass leaves the filter planes marked valid; the
    recording must contain their refresh all the same, or every replay convolves with the planes of the weights as they
    were before the recorded step.
    Before the recorders started from Network.mark_params_changed() both modes failed here: the loss of step 4 (the first
    replay) differed from the eager run's, and after step 6 the parameters were off by up to 4.99e-3, the moving statistics
    by 2.28."""
    monkeypatch.setenv("YOLO_STEP_MODE", mode)
    b1, b2 = data["b1"], data["b2"]

    def scenario(m, kinds):
        losses = [_step(m, b1, kinds), _step(m, b1, kinds)]
        outs = [o.clone() for o in m.net.forward(b2[0], training=False)]
        losses += [_step(m, b, kinds) for b in (b1, b2, b1, b2)]
        return losses, outs
    m = _run_both(scenario, [E, E, R, P, P, P])
    if mode == "graph":
        assert len(m._step_graphs.segments) == 1
    else:
        got = _names(m)
        assert got == clean_names, sorted((k, v, clean_names[k]) for k, v in (got | clean_names).items()
                                          if got[k] != clean_names[k])
        assert got["yolo_split_planes_batch"] > 0 and got["yolo_filter_transpose_batch"] > 0


def test_training_mode_forward_without_backward_before_the_recording(monkeypatch, data, clean_names):
    """T, T, model(x, training=True), T (records), T, T, T: a training-mode forward without backward marks the filter
    planes, the transposed filters and their planes valid and leaves the event of the second stream pending. Without the
    invalidation in front of the recording: first differing loss at step 4, parameters off by up to 4.99e-3 after step 6."""
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    b1, b2 = data["b1"], data["b2"]

    def scenario(m, kinds):
        losses = [_step(m, b1, kinds), _step(m, b1, kinds)]
        outs = m(b2[0], training=True)
        losses += [_step(m, b, kinds) for b in (b1, b2, b1, b2)]
        return losses, outs
    m = _run_both(scenario, [E, E, R, P, P, P])
    got = _names(m)
    assert got == clean_names, sorted((k, v, clean_names[k]) for k, v in (got | clean_names).items()
                                      if got[k] != clean_names[k])


def test_inference_between_replays(monkeypatch, data):
    """T x3, T, test_on_batch, T, predict (the captured inference graph of Network.infer), T, T: inference after replays
    sees the new weights, the folded BatchNorm scales and the moving statistics, and the replays after it are unharmed"""
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    b1, b2 = data["b1"], data["b2"]
    x, ys = data["x"], data["ys"]

    def scenario(m, kinds):
        losses = [_step(m, b, kinds) for b in (b1, b1, b1, b2)]
        tb = m.test_on_batch(x[4:8], [a[4:8] for a in ys])
        losses.append(_step(m, b1, kinds))
        pred = m.predict(x[8:12], batch_size=4)
        assert 4 in m.net._infer_graphs                   # (predict went through the captured inference graph)
        losses += [_step(m, b, kinds) for b in (b2, b1)]
        return losses + [tb], list(pred)
    _run_both(scenario, [E, E, R, P, P, P, P])


def test_batch_size_change_and_back(monkeypatch, data):
    """T x4 at batch 4, one T at batch 2 (Network.allocate re-allocates, alloc_gen moves), T x5 at batch 4: two eager steps,
    a second recording on the new buffers, two replays"""
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    b1, b2, small = data["b1"], data["b2"], data["small"]
    keys = []

    def scenario(m, kinds):
        losses = [_step(m, b, kinds) for b in (b1, b1, b1, b2)]
        if m._step_graphs is not None:
            keys.append(m._step_graphs.key)
        losses.append(_step(m, small, kinds))
        losses += [_step(m, b, kinds) for b in (b1, b2, b1, b2, b1)]
        return losses, []
    m = _run_both(scenario, [E, E, R, P, E, E, E, R, P, P])
    assert len(keys) == 1 and m._step_graphs.key != keys[0]


def test_weights_written_between_replays(monkeypatch, data):
    """T x4, set_weights on one conv layer (scaled by 0.5) and one BatchNorm layer, T x3: parameter storage does not move,
    so the recording stays in use and its replays read what was written"""
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    b1, b2 = data["b1"], data["b2"]
    recs = []

    def scenario(m, kinds):
        losses = [_step(m, b, kinds) for b in (b1, b1, b1, b2)]
        recs.append(m._step_graphs)
        conv, bn = m.get_layer("block5_4_3x3_conv"), m.get_layer("block5_4_3x3_bn")
        conv.set_weights([a * 0.5 for a in conv.get_weights()])
        gamma, beta, mean, var = bn.get_weights()
        bn.set_weights([gamma * 1.5, beta + 0.25, mean + 0.125, var * 2.0])
        losses += [_step(m, b, kinds) for b in (b1, b2, b1)]
        return losses, []
    m = _run_both(scenario, [E, E, R, P, P, P, P])
    assert m._step_graphs is recs[1]


def test_eager_step_between_replays(monkeypatch, data):
    """T x4, one step with metrics (which bypasses the recording), T x3"""
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    b1, b2 = data["b1"], data["b2"]

    def scenario(m, kinds):
        losses = [_step(m, b, kinds) for b in (b1, b1, b1, b2)]
        losses.append(_step(m, b1, kinds, with_metrics=True))
        losses += [_step(m, b, kinds) for b in (b2, b1, b2)]
        return losses, []
    _run_both(scenario, [E, E, R, P, E, P, P, P])


def _log_session(monkeypatch, log):
    """instrument (for the run that follows) what a session did: every training step as eager / record / replay, every
    evaluate as "eval" """
    from tf2_yolo_amd import capture
    from tf2_yolo_amd.model import Model

    def logged(cls, attr, token, replace_last):
        orig = getattr(cls, attr)

        def f(self, *a, **k):
            if replace_last:
                log[-1] = token
            else:
                log.append(token)
            return orig(self, *a, **k)
        monkeypatch.setattr(cls, attr, f)
    logged(Model, "train_step_device", E, False)
    logged(Model, "evaluate", "eval", False)
    logged(capture.StepTape, "__init__", R, True)
    logged(capture.StepTape, "replay", P, True)


@pytest.mark.parametrize("case", ["A", "B"])
def test_fit_with_validation_on_the_recorded_path(case, monkeypatch, data):
    """Model.fit with validation data, default step mode against YOLO_STEP_MODE=eager (fit seeds its own shuffle: both runs
    see the same batches). A: 8 rows in batches of 4, 4 epochs -- two eager steps, evaluate, the recording, replays with an
    evaluate after every second one. B: 14 rows in batches of 4, 4, 4, 2, 3 epochs -- the third step of every epoch records,
    the partial batch and the validation batch re-allocate, so every epoch makes a fresh recording. Without the
    invalidation in front of the recording A failed (the step recorded right after evaluate): mean loss of epoch 2 854.44
    against 799.69 eager, parameters off by up to 7.77e-3 after four epochs; B passed."""
    x, ys = data["x"], data["ys"]
    n, epochs = (8, 4) if case == "A" else (14, 3)
    val = (x[:4], [a[:4] for a in ys])
    res = {}
    for mode in ("eager", None):
        with monkeypatch.context() as mp:
            if mode is None:
                mp.delenv("YOLO_STEP_MODE", raising=False)
            else:
                mp.setenv("YOLO_STEP_MODE", mode)
            log = []
            _log_session(mp, log)
            m = _make()
            h = m.fit(x[:n], [a[:n] for a in ys], batch_size=4, epochs=epochs, validation_data=val, verbose=0).history
            res[mode] = (h["loss"] + h["val_loss"], _final(m), [])
        if mode == "eager":
            assert set(log) == {E, "eval"} and m._step_graphs is None
        elif case == "A":
            assert log == [E, E, "eval", R, P, "eval"] + [P, P, "eval"] * 2, log
            assert m._step_graphs is not None
        else:
            assert log == [E, E, R, E, "eval"] * 3, log
    assert len(res[None][0]) == 2 * epochs
    _compare(res["eager"], res[None])
