"""Model.predict in both inference precisions, same process, interleaved: YOLOv3-416 (C = 80) at batch 1 and 32, YOLOv4-608
(C = 80) at batch 16, synthetic weights (labels.synthetic_keras_weights, seed 1234, residual gamma 0.1: config 5's recipe).
Every round times fp32, fp16, fp32 again -- the two fp32 runs give the run-to-run spread the fp16 figure is read against.
Two clocks per run: `predict` = Model.predict on a host array (copies included, host clock around a synchronising call),
`infer` = Network.infer on a device-resident batch (device events around the graph replays).
usage: infer_precision_ab.py [rounds] [out.json]      -> profiles/infer_fp16_ab.json"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tf2_yolo_amd import graphs, labels

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "infer_fp16_ab.json")
CONFIGS = [("yolov3-416 c80", 3, 416, 1, 40), ("yolov3-416 c80", 3, 416, 32, 6), ("yolov4-608 c80", 4, 608, 16, 4)]


def build(version, hw):
    names = [f"c{i}" for i in range(80)]
    if version == 3:
        import yolov3
        y, g = yolov3.Yolo((hw, hw, 3), names), graphs.build_yolov3((hw, hw, 3), 80)
        y.create_model(pretrained_body=None)
    else:
        import yolov4
        y, g = yolov4.Yolo((hw, hw, 3), names), graphs.build_yolov4((hw, hw, 3), 80)
        y.create_model(anchors=graphs.V4_DEFAULT_ANCHORS, pretrained_body=None)
    w = labels.synthetic_keras_weights(g, 1234, residual_gamma=0.1)
    m = y.model
    for n in m.layer_names():
        lay = m.get_layer(n)
        k = len(lay.get_weights())
        if k and not n.endswith("_anchor"):
            lay.set_weights([w[f"{n}/{i}"] for i in range(k)])
    return m


def time_predict(m, x, bs, precision, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.predict(x, batch_size=bs, precision=precision)      # (ends in device-to-host copies: synchronises)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def time_infer(m, xd, precision, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        m.net.infer(xd, precision=precision)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    results = []
    models = {}
    for name, version, hw, bs, reps in CONFIGS:
        m = models.get((version, hw))
        if m is None:
            models.clear()
            torch.cuda.empty_cache()
            m = models[(version, hw)] = build(version, hw)
        x = np.random.default_rng(1234).random((bs, hw, hw, 3), dtype=np.float32)
        xd = torch.from_numpy(x).cuda()
        p32 = m.predict(x, batch_size=bs)                      # warm-up of both graphs, and the outputs' distance
        p16 = m.predict(x, batch_size=bs, precision="fp16")
        dist = max(float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(p32, p16))
        for prec in ("fp32", "fp16"):
            time_predict(m, x, bs, prec, 2)
            time_infer(m, xd, prec, 2)
        rows = {k: {"fp32_a": [], "fp16": [], "fp32_b": []} for k in ("predict_ms", "infer_ms")}
        for _ in range(ROUNDS):
            for slot, prec in (("fp32_a", "fp32"), ("fp16", "fp16"), ("fp32_b", "fp32")):
                rows["predict_ms"][slot].append(time_predict(m, x, bs, prec, reps))
                rows["infer_ms"][slot].append(time_infer(m, xd, prec, reps * 3))
        rec = {"config": name, "input": hw, "batch": bs, "rounds": ROUNDS, "reps_per_run": reps,
               "fp16_vs_fp32_output_distance": dist}
        for k, r in rows.items():
            a, h, b = (statistics.median(r[s]) for s in ("fp32_a", "fp16", "fp32_b"))
            f32 = 0.5 * (a + b)
            rec[k] = {"fp32_a": a, "fp16": h, "fp32_b": b, "fp32_spread": abs(a - b),
                      "fp32_spread_worst_round": max(abs(p - q) for p, q in zip(r["fp32_a"], r["fp32_b"])),
                      "fp32_over_fp16": f32 / h, "fp16_minus_fp32": h - f32, "runs": r}
        # acceptance: fp16 not slower than fp32 (mean of its two runs) by more than the spread between those two runs
        rec["fp16_within_fp32_spread"] = {k: rec[k]["fp16_minus_fp32"] <= rec[k]["fp32_spread"] for k in rows}
        print(json.dumps({k: v for k, v in rec.items() if k not in ("predict_ms", "infer_ms")} |
                         {k: {s: round(v, 4) for s, v in rec[k].items() if s != "runs"} for k in ("predict_ms", "infer_ms")}), flush=True)
        results.append(rec)
    out = {"device": torch.cuda.get_device_name(0), "what": __doc__.split("usage")[0].strip(), "results": results}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
