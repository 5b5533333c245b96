"""BASELINE config 5 end to end: YOLOv3-416 (C = 80) Model.predict at batch 1 -- the hipGraph replay of the inference
path built for few output pixels (csrc/conv_small.hip, the heads in one call, the Concatenate that reads through
UpSampling2D, the one-pass units with planes scaled from the a-priori bound) -- against the float64 oracle
(oracle/models.py), then decode and the three NMS modes on the device's own prediction against oracle/tools.py; the
same predict under every switch of that path (in-process for the ones the engine reads when a network is built, in
child processes for the launch policy the library reads once), after weight and batch-size changes, and YOLOv4-608 at
batch 1 (C = 20: the head's 64 x 64 tile at Cout 75, the Mish one-pass units, the four-source SPP concat).

Bar of every predict: each output within max(1e-4, 1.5 x the error of an fp32 CPU execution of the oracle on the same
network and image) of the float64 oracle, relative to the output's largest entry (test_gpu_model.test_model_parity)."""
import gc
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import infer_bs1_worker as W
from oracle import models as OM
from oracle import tools as T
from test_gpu_model import _rel, log_parity_ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
C5_TIMING = os.path.join(HERE, "golden", "tools_timing.json")


def _oracle(fwd, w, x, dtype):
    with torch.no_grad():
        outs = fwd({k: torch.tensor(v, dtype=dtype) for k, v in w.items()}, torch.tensor(x, dtype=dtype))
    return [o.numpy() for o in outs]


def _v3_fwd(w, x):
    from tf2_yolo_amd import graphs
    return OM.yolov3_forward(w, x, graphs.V3_DEFAULT_ANCHORS, training=False)[0]


def _v4_fwd(w, x):
    from tf2_yolo_amd import graphs
    return OM.yolov4_forward(w, x, graphs.V4_DEFAULT_ANCHORS, training=False)[0]


def _assert_parity(pred, ref, floor, case):
    """every output within max(1e-4, 1.5 floor) of the float64 oracle; logs the device / fp32-CPU error ratio"""
    bar = max(1e-4, 1.5 * floor)
    errs = []
    for a, b in zip(pred, ref):
        assert a.shape == b.shape and np.isfinite(a).all(), (case, a.shape, b.shape)
        errs.append(float(_rel(a, b)))
    log_parity_ratio({"case": case, "fp32_floor": float(floor), "forward_err": max(errs), "forward_ratio": max(errs) / max(floor, 1e-30)})
    assert max(errs) < bar, (case, errs, bar)


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def c5():
    """the network's weights, the image, the float64 oracle's prediction and the fp32 CPU floor -- once per module"""
    import conftest
    conftest.foreground_threads()
    w, x = W.c5_weights(), W.c5_image()
    o64 = _oracle(_v3_fwd, w, x, torch.float64)
    o32 = _oracle(_v3_fwd, w, x, torch.float32)
    floor = max(_rel(a, b) for a, b in zip(o32, o64))
    return {"w": w, "x": x, "o64": o64, "o32": o32, "floor": floor}


@pytest.fixture(scope="module")
def c5_pred(c5):
    """Model.predict at bs 1 under the default switches (hipGraph replay)"""
    m = W.build_c5(c5["w"])
    pred = m.predict(c5["x"], batch_size=1)
    del m
    _free()
    return pred


def test_c5_predict_matches_fp64_oracle(c5, c5_pred):
    """predict vs the float64 oracle; the graph replay bit-identical to the eager inference forward, and to itself"""
    _assert_parity(c5_pred, c5["o64"], c5["floor"], "C5 v3-416 c80 bs1 predict")
    m = W.build_c5(c5["w"])
    net = m.net
    xd = torch.from_numpy(c5["x"]).cuda()
    r1 = [o.clone() for o in net.infer(xd)]
    r2 = [o.clone() for o in net.infer(xd)]
    e = [o.clone() for o in net.forward(xd, training=False)]
    torch.cuda.synchronize()
    assert net._use_infer_graph and 1 in net._infer_graphs
    for a, b, c, p in zip(r1, r2, e, c5_pred):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert np.array_equal(a.cpu().numpy(), p)
    del m, net
    _free()


def _levels(pred):
    return [pred[2][0], pred[1][0], pred[0][0]]      # README.md: fine -> coarse


def test_c5_decode_and_nms_on_the_device_prediction(c5_pred):
    """decode_device at conf 0.5 on the device's own prediction bit-identical to oracle/tools.decode of the same arrays,
    and the three NMS modes on those candidates bit-identical to oracle/tools.py (the CPU NMS runs once, here)"""
    from tf2_yolo_amd import tools
    lv = _levels(c5_pred)
    dec = tools.decode_device(*[torch.from_numpy(a).cuda() for a in lv], class_num=80, threshold=0.5, version=3).cpu().numpy()
    ref = T.decode(*lv, class_num=80, threshold=0.5, version=3)
    assert dec.shape[0] > 40000 and np.array_equal(dec, ref)
    t0 = time.perf_counter()
    for name, got, want in (
            ("nms", lambda: tools.nms(dec, class_num=80, nms_threshold=0.5), lambda: T.nms(ref, 80, 0.5)),
            ("diou_nms", lambda: tools.nms(dec, class_num=80, nms_threshold=0.5, iou_mode=2), lambda: T.nms(ref, 80, 0.5, 2)),
            ("soft_nms", lambda: tools.soft_nms(dec, class_num=80, nms_threshold=0.5, conf_threshold=0.5, sigma=0.5),
             lambda: T.soft_nms(ref, 80, 0.5, 0.5, 0.5))):
        g, r = got(), want()
        print(f"C5 {name}: {dec.shape[0]} candidates, {g.shape[0]} kept")
        assert g.shape[0] > 0 and np.array_equal(g, r), name
    print(f"C5 oracle decode + three NMS modes on the CPU: {time.perf_counter() - t0:.1f} s")


def _joint_conf(level, C=80):
    """conf x class probability per (cell, anchor, class), in the level's dtype: what decode thresholds"""
    v = level.reshape(*level.shape[:2], -1, 5 + C)
    return v[..., 4:5] * v[..., 5:]


def test_c5_candidates_vs_fp64_oracle_and_the_golden_counts(c5, c5_pred):
    """The device's candidate set (joint confidence >= 0.5, the product decode forms in float32) equals the set of the
    float64 oracle's prediction except for rows whose float64 confidence lies within the measured forward error of 0.5;
    and the candidate count tests/golden/tools_timing.json quotes (decoded from the fp32 CPU oracle's prediction, not the
    device's) differs from the device's by at most the number of such near-threshold rows. The NMS kept counts are
    printed beside the golden ones: a few boxes a hair apart may change the suppression walk, so they are not asserted."""
    import json
    from tf2_yolo_amd import tools
    # measured error of the confidence / class outputs (the sigmoid channels), device and fp32 CPU, against float64
    def sig(o):
        return o.reshape(*o.shape[:3], -1, 85)[..., 4:]
    e = max(float(np.abs(sig(a) - sig(r)).max()) for d, c, r in zip(c5_pred, c5["o32"], c5["o64"]) for a in (d, c))
    assert e < 1e-4, e
    band = 2 * e + 2.0 ** -23          # |c p - c' p'| <= |c - c'| p + c' |p - p'|, plus the float32 product's rounding
    n_dev = n_ref = n_near = 0
    for dev, o64 in zip(c5_pred, c5["o64"]):
        jd, jr = _joint_conf(dev[0]), _joint_conf(o64[0])
        md, mr = jd >= np.float32(0.5), jr >= 0.5
        near = np.abs(jr - 0.5) <= band
        assert not (md != mr)[~near].any()
        n_dev, n_ref, n_near = n_dev + int(md.sum()), n_ref + int(mr.sum()), n_near + int(near.sum())
    dec = tools.decode(*_levels(c5_pred), class_num=80, threshold=0.5, version=3)
    assert dec.shape[0] == n_dev
    gold = json.load(open(C5_TIMING))["model_output"]
    kept = {k: int(tools.nms(dec, class_num=80, nms_threshold=0.5, iou_mode=m).shape[0])
            for k, m in (("nms_kept", 1), ("diou_nms_kept", 2))}
    kept["soft_nms_kept"] = int(tools.soft_nms(dec, class_num=80, nms_threshold=0.5, conf_threshold=0.5, sigma=0.5).shape[0])
    print(f"C5 candidates: device {n_dev}, float64 oracle {n_ref}, golden (fp32 CPU) {gold['candidates']}; rows within "
          f"{band:.3g} of the threshold: {n_near}; kept device / golden: " +
          ", ".join(f"{k} {v} / {gold[k]}" for k, v in kept.items()))
    assert abs(gold["candidates"] - n_dev) <= n_near
    assert abs(n_ref - n_dev) <= n_near


PY_SWITCHES = [{"YOLO_INFER_GRAPH": "0"}, {"YOLO_INFER_FUSE": "0"}, {"YOLO_INFER_ONEPASS": "0"},
               {"YOLO_INFER_SMALL_FUSE": "0"}, {"YOLO_CONCAT_PLANES": "0"},
               {"YOLO_INFER_ONEPASS": "0", "YOLO_INFER_SMALL_FUSE": "0"}]
_ATTR = {"YOLO_INFER_GRAPH": "_use_infer_graph", "YOLO_INFER_FUSE": "_fuse_infer", "YOLO_INFER_ONEPASS": "_infer_onepass",
         "YOLO_INFER_SMALL_FUSE": "_infer_small_fuse", "YOLO_CONCAT_PLANES": "_concat_planes"}


def _env_id(env):
    return " ".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.parametrize("env", PY_SWITCHES, ids=_env_id)
def test_c5_predict_under_engine_switches(c5, env, monkeypatch):
    """the switches engine.Network reads when it is built, set before create_model: predict vs the same float64 oracle"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = W.build_c5(c5["w"])
    for k in env:
        assert not getattr(m.net, _ATTR[k]), k
    pred = m.predict(c5["x"], batch_size=1)
    del m
    _free()
    _assert_parity(pred, c5["o64"], c5["floor"], f"C5 v3-416 c80 bs1 predict {_env_id(env)}")


LIB_SWITCHES = [{"YOLO_CONV_SMALL": "0"}, {"YOLO_CONV_SMALL": "3"},
                {"YOLO_CONV_SMALL": "3", "YOLO_CONV_SMALL_TILE": "21"},
                {"YOLO_CONV_SMALL": "3", "YOLO_CONV_SMALL_TILE": "22"}]


def _run_child(args, env_set, timeout, what):
    """one child process under a time limit; any failure ends the test before another child starts"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("YOLO_CONV_SMALL")}
    env.update(env_set)
    try:
        r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as ex:
        err = ex.stderr.decode(errors="replace") if isinstance(ex.stderr, bytes) else (ex.stderr or "")
        pytest.fail(f"{what} under {_env_id(env_set)}: no result within {timeout} s\n{err[-3000:]}")
    if r.returncode != 0:
        pytest.fail(f"{what} under {_env_id(env_set)}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return r


def test_c5_library_switches_in_child_processes(c5, tmp_path):
    """The launch policy of csrc/conv_small.hip is read once per process (C++ statics): under each setting a child
    process runs the bs-1 predict (tests/infer_bs1_worker.py), compared here with the module's float64 oracle; under the
    three YOLO_CONV_SMALL=3 settings -- every 3x3 unit through conv_small, the policy's tile or the 32 x 64 / 64 x 64 tile
    forced -- a second child runs the inference-unit tests of tests/test_gpu_conv.py (stride 2, 'valid', several images)."""
    shapes = [o.shape for o in c5["o64"]]
    for i, env_set in enumerate(LIB_SWITCHES):
        out = tmp_path / f"pred{i}.npy"
        _run_child([os.path.join(HERE, "infer_bs1_worker.py"), str(out)], env_set, 300, "bs-1 predict")
        flat = np.load(out)
        assert flat.size == sum(int(np.prod(s)) for s in shapes)
        pred, o = [], 0
        for s in shapes:
            n = int(np.prod(s))
            pred.append(flat[o:o + n].reshape(s))
            o += n
        _assert_parity(pred, c5["o64"], c5["floor"], f"C5 v3-416 c80 bs1 predict {_env_id(env_set)}")
        if env_set.get("YOLO_CONV_SMALL") == "3":
            r = _run_child(["-m", "pytest", os.path.join(HERE, "test_gpu_conv.py"), "-m", "gpu", "-q", "-x",
                            "-k", "inference_unit or random_shapes or head_unit"], env_set, 600, "test_gpu_conv.py")
            print(f"{_env_id(env_set)}: {r.stdout.strip().splitlines()[-1]}")


def test_c5_predict_after_weight_and_batch_changes(c5):
    """predict after set_weights raised one unit's gamma 4x (its a-priori bound K grows: a stale {K, D} would let the
    fp16 planes overflow) and cut another's moving variance to a quarter (a stale folded scale), against the float64
    oracle of the NEW weights; then three images at batch_size 2 (chunks of 2 and 1), then batch 1 again"""
    w, x = dict(c5["w"]), c5["x"]
    m = W.build_c5(w)
    _assert_parity(m.predict(x, batch_size=1), c5["o64"], c5["floor"], "C5 bs1 predict before the weight change")
    g_name, v_name = "block3_4_3x3_bn", "block4_3_1x1_bn"    # a 52x52 3x3 and a 26x26 1x1 unit, both through conv_small
    lay = m.get_layer(g_name)
    gw = lay.get_weights()
    gw[0] = gw[0] * 4
    lay.set_weights(gw)
    lay = m.get_layer(v_name)
    vw = lay.get_weights()
    vw[3] = vw[3] * 0.25
    lay.set_weights(vw)
    w[f"{g_name}/0"], w[f"{v_name}/3"] = gw[0], vw[3]
    x3 = np.concatenate([x, np.random.default_rng(99).random((2, 416, 416, 3), dtype=np.float32)])
    o64 = _oracle(_v3_fwd, w, x3, torch.float64)
    assert min(_rel(a[:1], b) for a, b in zip(o64, c5["o64"])) > 1e-3      # the change moves every output
    one = [o[:1] for o in o64]
    _assert_parity(m.predict(x, batch_size=1), one, c5["floor"], "C5 bs1 predict after the weight change")
    _assert_parity(m.predict(x3, batch_size=2), o64, c5["floor"], "C5 3 images at batch_size 2 after the weight change")
    _assert_parity(m.predict(x, batch_size=1), one, c5["floor"], "C5 bs1 predict after the batch-2 predict")
    del m
    _free()


@pytest.fixture(scope="module")
def v4_608():
    """YOLOv4-608, C = 20: synthetic_keras_weights(seed 1234, residual_gamma 0.1) -- the recipe of config 5 (with residual
    gamma 1 the float64 oracle's outputs overflow), image rng(1234); float64 oracle and fp32 CPU floor"""
    import conftest
    from tf2_yolo_amd import graphs, labels
    conftest.foreground_threads()
    w = labels.synthetic_keras_weights(graphs.build_yolov4((608, 608, 3), 20), 1234, residual_gamma=0.1)
    x = np.random.default_rng(1234).random((1, 608, 608, 3), dtype=np.float32)
    o64 = _oracle(_v4_fwd, w, x, torch.float64)
    o32 = _oracle(_v4_fwd, w, x, torch.float32)
    return {"w": w, "x": x, "o64": o64, "floor": max(_rel(a, b) for a, b in zip(o32, o64))}


@pytest.mark.parametrize("env", [{}, {"YOLO_INFER_SMALL_FUSE": "0"}], ids=lambda e: _env_id(e) or "default")
def test_v4_608_bs1_predict_matches_fp64_oracle(v4_608, env, monkeypatch):
    """YOLOv4-608 at bs 1: the 76x76 head (Cout 75) on the 64 x 64 tile, the Mish one-pass units, the SPP concat"""
    import yolov4
    from tf2_yolo_amd import graphs
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    y = yolov4.Yolo((608, 608, 3), [f"c{i}" for i in range(20)])
    y.create_model(anchors=graphs.V4_DEFAULT_ANCHORS, pretrained_body=None)
    W.set_weights(y.model, v4_608["w"])
    pred = y.model.predict(v4_608["x"], batch_size=1)
    del y
    _free()
    _assert_parity(pred, v4_608["o64"], v4_608["floor"], f"v4-608 c20 bs1 predict {_env_id(env) or 'default'}")
