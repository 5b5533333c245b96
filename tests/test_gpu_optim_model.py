"""Model level: clipping, momentum SGD and schedules inside real training steps -- eager, on the launch tape and in hipGraphs.

The model is the one of test_gpu_step_recording.py (YOLOv3 96x96, 8 classes = 39 head channels: every filter gradient runs
on the atomics-free kernels, so a step is bit-reproducible), batch 4, two different batches alternating after the
recording. Bars: losses equal to 1e-12 * max(|loss|, 1) (an fp64 sum whose atomics may change order); parameters,
BatchNorm moving statistics and every optimizer slot bit-identical. Every case pins which steps were eager, which one
recorded and which replayed, and that the clipping threshold really bit."""
import collections
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A9 = [[0.89663461, 0.78365384], [0.375, 0.47596153], [0.27884615, 0.21634615], [0.14182692, 0.28605769],
      [0.14903846, 0.10817307], [0.07211538, 0.14663461], [0.07932692, 0.05528846], [0.03846153, 0.07211538],
      [0.02403846, 0.03125]]
HW, CLASSES = 96, 8
E, R, P = "eager", "record", "replay"
NEW_CALLS = {"yolo_grad_sqnorm", "yolo_clip_factors", "yolo_adam_step_clip", "yolo_sgd_step_clip"}


def _make(optimizer, recording=True):
    import yolov3
    y = yolov3.Yolo((HW, HW, 3), list("abcdefgh"))
    y.create_model(anchors=A9, pretrained_body=None, seed=11)
    y.model.compile(optimizer=optimizer, loss=y.loss())
    y.model._graphs_failed = not recording       # eager reference: the switch a failed recording would flip
    return y.model


@pytest.fixture(scope="module")
def data():
    """two device batches of 4; never modified"""
    from tf2_yolo_amd import labels
    x, ys = labels.synthetic_batch(np.random.default_rng(3), 8, (HW, HW), CLASSES)
    dev = lambda sl: (torch.from_numpy(x[sl]).cuda(), [torch.from_numpy(a[sl]).cuda() for a in ys])
    return {"b1": dev(slice(0, 4)), "b2": dev(slice(4, 8))}


@pytest.fixture(scope="module")
def first_norm(data):
    """global gradient norm of the first step, from a throw-away model whose threshold is never reached; and the number of
    variables of the model"""
    from tf2_yolo_amd.optimizers import Adam
    m = _make(Adam(learning_rate=1e-3, global_clipnorm=1e30), recording=False)
    assert m.optimizer.last_grad_norm() is None          # no step yet
    m.train_step_device(*data["b1"])
    n = m.optimizer.last_grad_norm()
    assert n is not None and math.isfinite(n) and n > 0
    return n, len(m.net.params.order)


def _step(m, batch, kinds):
    """one training step; appends what it was (eager / record / replay) to `kinds`, returns the per-output losses"""
    g0 = m._step_graphs
    bufs, _ = m.train_step_device(*batch)
    g1 = m._step_graphs
    kinds.append(E if g1 is None else P if g1 is g0 else R)
    return [float(b[0].item()) for b in bufs]


def _final(m):
    torch.cuda.synchronize()
    out = {"params": m.net.params.data, "state": m.net.state.data}
    out.update({"slot " + k: v for k, v in m.optimizer.slots().items()})
    return {k: v.clone() for k, v in out.items()}


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(abs(a), 1.0)


def _run(optimizer, batches, recording=True, norms=None):
    m = _make(optimizer, recording)
    kinds, losses = [], []
    for b in batches:
        losses.append(_step(m, b, kinds))
        if norms is not None:
            norms.append(m.optimizer.last_grad_norm())
    return m, kinds, losses, _final(m)


def _assert_same(ref, got, what):
    (l0, f0), (l1, f1) = ref, got
    first = next((i + 1 for i, (a, b) in enumerate(zip(l0, l1)) if not all(_close(u, v) for u, v in zip(a, b))), None)
    diffs = {k: float((f0[k].double() - f1[k].double()).abs().max()) for k in f0}
    print(f"\n[{what}] first step whose loss differs: {first}; max |diff| {diffs}")
    assert len(l0) == len(l1) and first is None, (first, l0, l1)
    assert f0.keys() == f1.keys()
    for k in f0:
        assert torch.equal(f0[k], f1[k]), k


def _optimizers(first_norm):
    """name -> (factory, threshold as a fraction of what last_grad_norm() reports). global_clipnorm: half the first step's
    norm. clipnorm: the largest variable has at least norm / sqrt(V) (the squares of V variables add up to norm^2), so half
    of THAT is exceeded by at least one variable whenever the global norm is at least the first step's.
    The rate of the SGD run is 1e-5: a clipped step moves the parameters by rate * threshold in norm, and the gradient of an
    untrained net with exp() box heads falls steeply along it -- at 1e-3 that is a move of ~5 per step and the norm is below
    half of the first step's from the second step on, so clipping would bite on the first step only; at 1e-5 the move is
    ~0.05 per step, and every step of the run, the replays included, is clipped."""
    from tf2_yolo_amd.optimizers import SGD, Adam
    n, nvars = first_norm
    t_global, t_var = 0.5 * n, 0.5 * n / math.sqrt(nvars)
    return {"adam_global": (lambda: Adam(learning_rate=1e-3, global_clipnorm=t_global), t_global, 1.0),
            "adam_clipnorm": (lambda: Adam(learning_rate=1e-3, clipnorm=t_var), t_var, 1.0 / math.sqrt(nvars)),
            "sgd_nesterov_global": (lambda: SGD(learning_rate=1e-5, momentum=0.9, nesterov=True, global_clipnorm=t_global),
                                    t_global, 1.0)}


@pytest.mark.parametrize("mode", ["tape", "graph"])
@pytest.mark.parametrize("opt", ["adam_global", "adam_clipnorm", "sgd_nesterov_global"])
def test_recorded_step_equals_eager_step(opt, mode, monkeypatch, data, first_norm):
    """E, E, R, P, P, P over two alternating batches against the same six steps through Python. The momentum-SGD run must
    record and replay (plain SGD never did). In tape mode the recording holds the new calls and not yolo_adam_step_dev."""
    monkeypatch.setenv("YOLO_STEP_MODE", mode)
    factory, threshold, share = _optimizers(first_norm)[opt]
    b1, b2 = data["b1"], data["b2"]
    batches = [b1, b1, b1, b2, b1, b2]
    norms_e, norms_r = [], []
    me, kinds_e, losses_e, final_e = _run(factory(), batches, recording=False, norms=norms_e)
    mr, kinds_r, losses_r, final_r = _run(factory(), batches, recording=True, norms=norms_r)
    assert set(kinds_e) == {E} and me._step_graphs is None
    assert kinds_r == [E, E, R, P, P, P], kinds_r
    print(f"\n[{opt} / {mode}] threshold {threshold:.4g}; global norms per step {norms_r}")
    # a run in which clipping never bit proves nothing: on a LATER step the norm (for clipnorm: the least the largest
    # variable can have, norm / sqrt(V)) exceeded the threshold
    assert any(n * share > threshold for n in norms_r[1:]), (norms_r, threshold)
    assert norms_e == norms_r
    _assert_same((losses_e, final_e), (losses_r, final_r), f"{opt} / {mode}: recorded vs eager")
    assert losses_r[2] != losses_r[3]                    # (b2 really went through the recording)
    assert any(k.startswith("slot ") for k in final_r)
    if mode == "graph":
        assert len(mr._step_graphs.segments) == 1
    else:
        names = collections.Counter(name for _, _, name in mr._step_graphs.tape.entries)
        update = "yolo_sgd_step_clip" if opt.startswith("sgd") else "yolo_adam_step_clip"
        assert names["yolo_grad_sqnorm"] == 1 and names["yolo_clip_factors"] == 1 and names[update] == 1
        assert names["yolo_adam_step_dev"] == 0 and names["yolo_adam_step"] == 0 and names["yolo_sgd_step"] == 0


def test_tape_of_a_plain_adam_step_holds_none_of_the_new_calls(monkeypatch, data):
    from tf2_yolo_amd.optimizers import Adam
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    m, kinds, _, _ = _run(Adam(learning_rate=1e-3), [data["b1"]] * 3)
    assert kinds == [E, E, R]
    names = collections.Counter(name for _, _, name in m._step_graphs.tape.entries)
    assert names["yolo_adam_step_dev"] == 1 and not (NEW_CALLS & set(names))
    assert m.optimizer.last_grad_norm() is None


def test_threshold_never_reached_equals_plain_adam(monkeypatch, data):
    """Adam(global_clipnorm=1e30) against Adam after six steps (two eager, the recording, three replays each): the factor
    is exactly 1 and the update kernel does adam_kernel's arithmetic, so no bit differs"""
    from tf2_yolo_amd.optimizers import Adam
    monkeypatch.delenv("YOLO_STEP_MODE", raising=False)
    b1, b2 = data["b1"], data["b2"]
    batches = [b1, b1, b1, b2, b1, b2]
    _, kinds_a, losses_a, final_a = _run(Adam(learning_rate=1e-3), batches)
    m, kinds_b, losses_b, final_b = _run(Adam(learning_rate=1e-3, global_clipnorm=1e30), batches)
    assert kinds_a == kinds_b == [E, E, R, P, P, P]
    _assert_same((losses_a, final_a), (losses_b, final_b), "global_clipnorm=1e30 vs plain Adam")
    assert m.optimizer.last_grad_norm() > 0


@pytest.mark.parametrize("mode", ["eager", "tape"])
def test_schedule_is_followed_inside_replays(mode, monkeypatch, data):
    """Adam(PiecewiseConstantDecay([3], [1e-3, 0.0])): the schedule sees steps 0, 1, 2, 3 at the first four steps (rate 1e-3)
    and 4 at the fifth (rate 0): from the fifth step on no parameter bit changes, eager or replayed"""
    from tf2_yolo_amd.optimizers import Adam
    from tf2_yolo_amd.optimizers.schedules import PiecewiseConstantDecay
    monkeypatch.setenv("YOLO_STEP_MODE", mode)
    m = _make(Adam(learning_rate=PiecewiseConstantDecay([3], [1e-3, 0.0])))
    kinds, after = [], []
    for b in [data["b1"], data["b1"], data["b1"], data["b2"], data["b1"], data["b2"], data["b1"]]:
        _step(m, b, kinds)
        after.append(m.net.params.data.clone())
    assert kinds == ([E] * 7 if mode == "eager" else [E, E, R, P, P, P, P])
    assert not torch.equal(after[2], after[3])           # the fourth step still moved the parameters
    assert all(torch.equal(after[3], a) for a in after[4:])
    assert m.optimizer.iterations == 7


def test_assigned_learning_rate_reaches_the_replays_of_momentum_sgd(monkeypatch, data):
    """`optimizer.lr = ...` between steps (what a LearningRateScheduler callback does from on_epoch_begin) takes effect at
    the next step, a replay included: same bits as the run in which every step goes through Python"""
    from tf2_yolo_amd.optimizers import SGD
    monkeypatch.setenv("YOLO_STEP_MODE", "tape")
    res = {}
    for recording in (False, True):
        m = _make(SGD(learning_rate=1e-3, momentum=0.9), recording)
        kinds, losses = [], []
        for i, b in enumerate([data["b1"], data["b1"], data["b1"], data["b2"], data["b1"]]):
            if i == 3:
                m.optimizer.lr = 0.0
            losses.append(_step(m, b, kinds))
            if i == 3:     # rate 0 from here on: the accumulator keeps decaying, and keeps moving the parameters
                p3, a3 = m.net.params.data.clone(), m.optimizer.a.clone()
        assert kinds == ([E, E, R, P, P] if recording else [E] * 5)
        assert torch.equal(m.optimizer.a, a3 * np.float32(0.9)) and not torch.equal(m.net.params.data, p3)
        res[recording] = (losses, _final(m))
    _assert_same(res[False], res[True], "momentum SGD with an assigned rate: recorded vs eager")


def test_global_norm_counts_the_trainable_anchors():
    """YOLOv4 with anchors_trainable (the configuration of test_gpu_keras_shell.py::test_v4_trainable_anchors) and
    SGD(1e-3, global_clipnorm=t): last_grad_norm()^2 = sum of squares of the parameter gradients AND the anchor gradients,
    to 1e-5 relative (the anchor gradient is an fp32 atomic sum). The gradients come from a twin model stepped with
    SGD(0.0) -- whose parameters therefore stay those of the first step -- and one more backward pass on it."""
    import yolov4
    from tf2_yolo_amd import labels
    from tf2_yolo_amd.optimizers import SGD
    x_h, ys_h = labels.synthetic_batch(np.random.default_rng(5), 4, (64, 64), 2)
    x = torch.from_numpy(x_h).cuda()
    ys = [torch.from_numpy(v).cuda() for v in ys_h]

    def make(optimizer):
        y = yolov4.Yolo((64, 64, 3), ["a", "b"])
        y.create_model(anchors=A9, pretrained_body=None)
        y.model.compile(optimizer=optimizer, loss=y.loss())
        y.anchors_trainable = True
        assert y.model.net.anchors_trainable
        return y.model

    twin = make(SGD(learning_rate=0.0))
    p0 = twin.net.params.data.clone()
    twin.train_step_device(x, ys)
    assert torch.equal(twin.net.params.data, p0) and float(twin.net.grads.abs().max()) == 0.0
    net = twin.net
    outs = net.forward(x, training=True)
    dpred = [torch.empty_like(o) for o in outs]
    for i, (o, yt) in enumerate(zip(outs, ys)):
        twin.loss[i].fwd_bwd(yt, o, grad_scale=1.0, dpred=dpred[i], loss_out=torch.zeros(8, device="cuda", dtype=torch.float64))
    net.backward(dpred)
    torch.cuda.synchronize()
    sq_p = float((net.grads.double() ** 2).sum())        # (the padding of the flat gradient buffer is never written: zero)
    sq_a = float((net.anchor_grads.double() ** 2).sum())
    assert sq_a > 0 and sq_p > 0
    want = math.sqrt(sq_p + sq_a)
    m = make(SGD(learning_rate=1e-3, global_clipnorm=0.5 * want))
    a0 = m.net.anchors_flat.clone()
    m.train_step_device(x, ys)
    got = m.optimizer.last_grad_norm()
    print(f"\n[anchors] norm^2 {got * got:.9g}; parameters {sq_p:.9g} + anchors {sq_a:.9g} = {sq_p + sq_a:.9g}")
    assert abs(got * got - (sq_p + sq_a)) <= 1e-5 * (sq_p + sq_a)
    # each of the two ordered sums on its own, so that the anchors' share is checked however small it is beside the other
    assert float(m.optimizer._table.total_sq[0]) == pytest.approx(sq_p, rel=1e-5)
    assert float(m.optimizer._anch.total_sq[0]) == pytest.approx(sq_a, rel=1e-5)
    assert not torch.equal(m.net.anchors_flat, a0)       # and the clipped step moved them


def test_one_rank_data_parallel_clips_the_same_bits():
    """enable_data_parallel on a process group of one rank (RCCL, set up as in test_gpu_dp.py: a fresh process that creates
    the step's streams before the process group) with global_clipnorm: six steps give the bits of the run without it.
    The worker is tests/dp_clip_worker.py."""
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29553", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", YOLO_DP_FORCE="1")     # (run the collectives in a world of one too)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dp_clip_worker.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:]
    j = json.loads(lines[-1])
    print("\n[one-rank DP]", j)
    assert j["kinds_plain"] == j["kinds_dp"] == [E, E, R, P, P, P]
    assert j["world"] == 1 and j["reducer_active"] is True
    assert any(n > j["threshold"] for n in j["norms_dp"][1:])
    assert j["norms_plain"] == j["norms_dp"]
    assert j["losses_equal"] and j["bit_identical"] == {"params": True, "state": True, "slot m": True, "slot v": True,
                                                        "slot anchors/m": True, "slot anchors/v": True}
