"""Training step of the darknet53 classifier (bodies.darknet53, 256 x 256, batch 32, 1000 classes, Adam) and the share of
it that the classifier top takes: GlobalAveragePooling2D, Dense + softmax, categorical cross-entropy and their backward
(csrc/classify.hip). A record, not a threshold: -> profiles/classifier_step.json (quoted in DESIGN.md).

  step_ms   device events around WINDOW recorded steps (the default step mode) after WARMUP steps; the median of REPEATS windows
  top_ms    device events around TOP_REPS back-to-back runs of the top's five library calls on the buffers the steps just
            used (same shapes, same pointers, scratch gradient slices), per run; the median of REPEATS windows. Back-to-back
            runs keep the 4 MB kernel of the Dense layer in cache, as it is not inside a step: the figure is a floor of the
            top's time in the step, and the share with it. top_calls_ms: each of the five calls alone, the same way.

usage: python scripts/classifier_step.py [--batch 32] [--size 256] [--classes 1000] [--out profiles/classifier_step.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402

WARMUP, WINDOW, REPEATS, TOP_REPS = 6, 20, 5, 200


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classifier_step.py measures on the GPU: no device found")
    from tf2_yolo_amd import bodies, ops, optimizers
    N, K = a.batch, a.classes
    m = bodies.darknet53(weights=None, input_shape=(a.size, a.size, 3), class_num=K)
    m.compile(optimizer=optimizers.Adam(learning_rate=1e-4), loss="categorical_crossentropy")
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((N, a.size, a.size, 3), dtype=np.float32)).cuda()
    t = torch.zeros((N, K), device="cuda")
    t[torch.arange(N), torch.from_numpy(rng.integers(0, K, N)).cuda()] = 1.0

    def step():
        m.train_step_device(x, [t])
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    recorded = m._step_graphs is not None
    step_ms = [timed(step, WINDOW) for _ in range(REPEATS)]
    loss = float(m._loss_bufs[0][0].item())

    net = m.net
    gap, dense = net.units[-2], net.units[-1]
    feat = net.act[gap.src.tid]
    w, b = net.params.view(dense.p_kernel.name), net.params.view(dense.p_bias.name)
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    dpred, lbuf = torch.empty_like(dense.buf), torch.zeros(8, device="cuda", dtype=torch.float64)

    calls = {
        "yolo_gap_fwd": lambda: ops.gap_fwd(feat, out=gap.buf),
        "yolo_dense_softmax_fwd": lambda: ops.dense_softmax_fwd(gap.buf, w, b, logits=dense.logits, p=dense.buf),
        "yolo_cce_fwd_bwd": lambda: ops.cce_fwd_bwd(t, dense.buf, loss_out=lbuf, dpred=dpred),
        "yolo_dense_softmax_bwd": lambda: ops.dense_softmax_bwd(dpred, dense.buf, gap.buf, w, dense.dsrc, dw=dw, db=db,
                                                                dz=dense.dz),
        "yolo_gap_bwd": lambda: ops.gap_bwd(dense.dsrc, gap.dsrc),
    }

    def top():
        for f in calls.values():
            f()
    timed(top, 10)
    top_ms = [timed(top, TOP_REPS) for _ in range(REPEATS)]
    each_ms = {name: round(statistics.median(timed(f, TOP_REPS) for _ in range(REPEATS)), 4) for name, f in calls.items()}
    s, tp = statistics.median(step_ms), statistics.median(top_ms)
    rec = {"model": "darknet53 classifier", "input": [a.size, a.size, 3], "batch": N, "class_num": K, "optimizer": "Adam",
           "device": torch.cuda.get_device_name(0), "step_recorded": recorded, "loss_after": loss,
           "step_ms": round(s, 3), "step_ms_windows": [round(v, 3) for v in step_ms], "images_per_s": round(N / s * 1e3, 1),
           "top_ms": round(tp, 4), "top_ms_windows": [round(v, 4) for v in top_ms], "top_share_of_step": round(tp / s, 5),
           "top_calls_ms": each_ms,
           "method": f"device events; step: median of {REPEATS} windows of {WINDOW} steps after {WARMUP} warm-up steps; top: "
                     f"median of {REPEATS} windows of {TOP_REPS} back-to-back runs of its five calls on the step's buffers; top_calls_ms: each call alone, the same way"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
