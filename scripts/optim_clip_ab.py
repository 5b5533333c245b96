"""What gradient clipping costs per step: YOLOv3-416, batch 32, Adam(1e-4) against Adam(1e-4, global_clipnorm=t), same
process, same box, two models from the same seed, blocks of K steps ALTERNATING between them (step mode as the environment
says: the launch tape by default). t = half the gradient norm of the first step, so the threshold bites.
usage: optim_clip_ab.py [--k K] [--rounds R] [--only plain|clip] [--hw 416] [--batch 32]
--only clip runs one model alone: the form to put behind a kernel trace (sqnorm_chunk_kernel, sqnorm_sum_kernel,
clip_factors_kernel, adam_clip_kernel are the four launches clipping puts in place of adam_kernel)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--only", choices=["plain", "clip"])
ap.add_argument("--hw", type=int, default=416)
ap.add_argument("--batch", type=int, default=32)
a = ap.parse_args()
from tf2_yolo_amd import labels, optimizers, ops
ops.create_side_streams()
import yolov3

x_h, ys_h = labels.synthetic_batch(np.random.default_rng(0), a.batch, (a.hw, a.hw), 80)
x = torch.from_numpy(x_h).cuda(); ys = [torch.from_numpy(t).cuda() for t in ys_h]


def make(**kw):
    y = yolov3.Yolo((a.hw, a.hw, 3), [f"c{i}" for i in range(80)])
    y.create_model(pretrained_body=None, seed=1234)
    y.model.compile(optimizer=optimizers.Adam(learning_rate=1e-4, **kw), loss=y.loss())
    return y.model


probe = make(global_clipnorm=1e30)
probe.train_step_device(x, ys)
threshold = 0.5 * probe.optimizer.last_grad_norm()
del probe
torch.cuda.empty_cache()
models = {}
if a.only != "clip":
    models["plain"] = make()
if a.only != "plain":
    models["clip"] = make(global_clipnorm=threshold)
for m in models.values():
    for _ in range(5):                  # two eager steps, the recording, two replays
        m.train_step_device(x, ys)
torch.cuda.synchronize()
times = {k: [] for k in models}
for r in range(a.rounds):
    for name, m in models.items():
        m.train_step_device(x, ys)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.k):
            m.train_step_device(x, ys)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / a.k * 1e3)
    print(f"round {r}: " + "   ".join(f"{n} {t[-1]:.3f}" for n, t in times.items()) + "  ms/step", flush=True)
out = {"config": f"yolov3-{a.hw} batch {a.batch}", "threshold": threshold, "k": a.k,
       "ms_per_step": {n: {"median": float(np.median(t)), "min": min(t), "max": max(t)} for n, t in times.items()}}
if "clip" in models:
    out["last_grad_norm"] = models["clip"].optimizer.last_grad_norm()
    out["chunks"] = models["clip"].optimizer._table.n_chunks
    out["variables"] = models["clip"].optimizer._table.n_vars
print(json.dumps(out), flush=True)
