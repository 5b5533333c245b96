"""Images in, boxes out, two ways in one process on one box: (a) Model.predict, then tools._detections image by image (every
head tensor to the host and its slices back up, about twenty launches and two host round trips per image) against (b)
Model.detect (decode + NMS of the whole chunk on the device, three host reads per chunk, only the kept rows come back).
YOLOv3-416 (C = 80), synthetic weights (labels.synthetic_keras_weights, seed 1234, residual gamma 0.1) on rng(1234) pixels,
batch 1 and 32, nms_mode 1 and 2, at conf_threshold 0.5 -- which on this network IS the dense case of
tests/golden/tools_timing.json (47 817 candidates in image 0) -- and at a second threshold: the one that gives about 47 817
candidates per image over the batch if 0.5 does not, else 0.9 (a sparse case beside the dense one).
Both paths must return equal arrays before anything is timed. Every round times (a) then (b): host clock around
synchronised calls, one untimed call after every switch of path, median and min / max over the rounds.
usage: detect_batch_ab.py [rounds] [out.json]      -> profiles/detect_batch_ab.json
       detect_batch_ab.py alone [out.json]        -> profiles/detect_batch_alone.json: Model.detect in a process that never
                                                     runs path (a) (same configurations, same clock)
       detect_batch_ab.py trace MODE              four batch-32 detect calls at 0.5 and nothing else, for
                                                     rocprofv3 --kernel-trace --stats (profiles/detect_batch_kernel_stats_mode*.csv)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tf2_yolo_amd import graphs, labels, tools

SUB = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("alone", "trace") else None
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and SUB is None else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "detect_batch_alone.json" if SUB else "detect_batch_ab.json")
HW, C, DENSE = 416, 80, 47817
NMS_THR, SIGMA = 0.45, 0.5
BATCHES = [(1, 10), (32, 5)]      # (batch, calls per timed run)


def build():
    import yolov3
    y, g = yolov3.Yolo((HW, HW, 3), [f"c{i}" for i in range(C)]), graphs.build_yolov3((HW, HW, 3), C)
    y.create_model(pretrained_body=None)
    w = labels.synthetic_keras_weights(g, 1234, residual_gamma=0.1)
    m = y.model
    for n in m.layer_names():
        lay = m.get_layer(n)
        k = len(lay.get_weights())
        if k:
            lay.set_weights([w[f"{n}/{i}"] for i in range(k)])
    return m


def path_a(m, x, bs, thr, mode):
    pred = m.predict(x, batch_size=bs)
    return [tools._detections([lv[b] for lv in pred], C, thr, mode, NMS_THR, SIGMA, 3) for b in range(len(x))]


def path_b(m, x, bs, thr, mode):
    return m.detect(x, batch_size=bs, conf_threshold=thr, nms_mode=mode, nms_threshold=NMS_THR, nms_sigma=SIGMA)


def timed(fn, calls):
    fn()      # untimed: the first call after the other path finds the caching allocator and the host buffers in that path's state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def products(pred):
    out = []
    for lv in pred:
        t = lv.reshape(*lv.shape[:3], 3, 5 + C)
        out.append((t[..., 4:5] * t[..., 5:]).reshape(lv.shape[0], -1))
    return np.concatenate(out, axis=1)


def alone(m):
    results = []
    for bs, calls in BATCHES:
        x = np.random.default_rng(1234).random((bs, HW, HW, 3), dtype=np.float32)
        for thr in (0.5, 0.9):
            for mode in (1, 2):
                timed(lambda: path_b(m, x, bs, thr, mode), 2)
                tb = [timed(lambda: path_b(m, x, bs, thr, mode), calls) for _ in range(ROUNDS)]
                rec = {"batch": bs, "conf_threshold": thr, "nms_mode": mode, "rounds": ROUNDS, "calls_per_run": calls,
                       "detect_alone_ms": {"median": statistics.median(tb), "min": min(tb), "max": max(tb)}}
                print(json.dumps(rec), flush=True)
                results.append(rec)
    return results


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    m = build()
    if SUB == "trace":
        x = np.random.default_rng(1234).random((32, HW, HW, 3), dtype=np.float32)
        for _ in range(4):
            path_b(m, x, 32, 0.5, int(sys.argv[2]))
        torch.cuda.synchronize()
        return
    if SUB == "alone":
        out = {"device": torch.cuda.get_device_name(0), "what": "Model.detect alone, no other path in the process; "
               "configurations and clock of detect_batch_ab.json", "results": alone(m)}
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", OUT)
        return
    results = []
    for bs, calls in BATCHES:
        x = np.random.default_rng(1234).random((bs, HW, HW, 3), dtype=np.float32)
        p = products(m.predict(x, batch_size=bs))
        at_half = float((p >= np.float32(0.5)).sum(axis=1).mean())
        if abs(at_half - DENSE) <= 0.1 * DENSE:
            second = 0.9
        else:   # the threshold with DENSE candidates per image on average: the (DENSE * bs)-th largest product
            second = float(np.partition(p.ravel(), -DENSE * bs)[-DENSE * bs])
        del p
        for thr in (0.5, second):
            for mode in (1, 2):
                a, b = path_a(m, x, bs, thr, mode), path_b(m, x, bs, thr, mode)
                assert len(a) == len(b) == bs and all(np.array_equal(p_, q_) for p_, q_ in zip(a, b)), (bs, thr, mode)
                cand = sum(r.shape[0] for r in path_b(m, x, bs, thr, 0))
                kept = sum(r.shape[0] for r in b)
                for fn in (path_a, path_b):
                    timed(lambda: fn(m, x, bs, thr, mode), 2)
                ta, tb = [], []
                for _ in range(ROUNDS):
                    ta.append(timed(lambda: path_a(m, x, bs, thr, mode), calls))
                    tb.append(timed(lambda: path_b(m, x, bs, thr, mode), calls))
                ma, mb = statistics.median(ta), statistics.median(tb)
                rec = {"batch": bs, "conf_threshold": thr, "nms_mode": mode, "candidates_per_image": cand / bs,
                       "kept_per_image": kept / bs, "rounds": ROUNDS, "calls_per_run": calls,
                       "predict_then_per_image_ms": {"median": ma, "min": min(ta), "max": max(ta)},
                       "detect_ms": {"median": mb, "min": min(tb), "max": max(tb)},
                       "speedup": ma / mb, "detect_slower": mb > ma}
                print(json.dumps(rec), flush=True)
                results.append(rec)
    out = {"device": torch.cuda.get_device_name(0), "what": __doc__.split("usage")[0].strip(), "results": results}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
