"""Raw uint8 images in, two ways in one process: (A) what a caller does without the device-side preparation --
`x_u8.astype(np.float32) * (1 / 255)` on the host, conversion INSIDE the timed region, then detect / predict / fit on the float32
array -- against (B) `detect_images(x_u8, rescale=1 / 255)` (tf2_yolo_amd/images.py: pinned uint8 staging, one H2D copy of a quarter of
the bytes, csrc/image.hip on the device). YOLOv3-416, C = 80, synthetic weights (labels.synthetic_keras_weights, seed 1234,
residual gamma 0.1), rng(1234) pixels, batch 1 and 32, conf_threshold 0.9. Both arms must return equal arrays before anything is
timed. Every round times (A) then (B): host clock around calls that end in a device synchronise, one untimed call after every
switch of arm, median and min / max over the rounds.
The fit arms (one epoch of 8 batches of 16 images, shuffle off, SGD) each run in a process of their own, because the peak
resident set of a process never falls: two untimed epochs (the step is recorded during them), then `rounds` timed epochs;
ru_maxrss at the end tells whether the float32 copy of the data set was ever made.
usage: image_input_ab.py [rounds] [out.json]            -> profiles/image_input_ab.json
       image_input_ab.py baseline [rounds] [out.json]   arm (A) alone: runs on a tree without the new keywords too (the
                                                        parent commit's figures in profiles/image_input_ab.json come from it)
       image_input_ab.py fit A|B [rounds]               one fit arm, one JSON line (started by the two forms above)
       image_input_ab.py trace                          four batch-32 prepare calls and nothing else, for
                                                        rocprofv3 --kernel-trace --stats"""
import json
import os
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tf2_yolo_amd import graphs, labels

ARGS = sys.argv[1:]
SUB = ARGS.pop(0) if ARGS and ARGS[0] in ("baseline", "fit", "trace") else None
FIT_ARM = ARGS.pop(0) if SUB == "fit" else None
ROUNDS = int(ARGS.pop(0)) if ARGS and ARGS[0].isdigit() else 5
OUT = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "image_input_ab.json")
HW, C, THR, S = 416, 80, 0.9, 1 / 255
BATCHES = [(1, 10), (32, 5)]      # (batch, calls per timed run)
FIT_BATCH, FIT_BATCHES = 16, 8


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
    return y, m


def host_f32(x):
    return x.astype(np.float32) * np.float32(S)


def timed(fn, calls):
    fn()      # untimed: the first call after the other arm finds the caching allocator and the host buffers in that arm's state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def listed(p):
    return p if isinstance(p, list) else [p]


def fit_arm(arm):
    from tf2_yolo_amd.optimizers import SGD
    y, m = build()
    m.compile(optimizer=SGD(learning_rate=1e-5), loss=y.loss())
    rng = np.random.default_rng(1234)
    n = FIT_BATCH * FIT_BATCHES
    _, ys = labels.synthetic_batch(rng, n, (HW, HW), C)
    x = rng.integers(0, 256, (n, HW, HW, 3), dtype=np.uint8)
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss

    def epoch():
        if arm == "A":
            m.fit(host_f32(x), ys, batch_size=FIT_BATCH, epochs=1, verbose=0, shuffle=False)
        else:
            m.fit(x, ys, batch_size=FIT_BATCH, epochs=1, verbose=0, shuffle=False, rescale=S)
        torch.cuda.synchronize()
    epoch(), epoch()
    ts = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        epoch()
        ts.append((time.perf_counter() - t0) * 1e3)
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps({"arm": arm, "epoch_ms": stats(ts), "loss": m.history.history["loss"][-1], "rounds": ROUNDS,
                      "peak_rss_mb_before_fit": rss0 / 1024, "peak_rss_mb": rss / 1024,
                      "uint8_mb": x.nbytes / 2 ** 20, "float32_mb": 4 * x.nbytes / 2 ** 20}), flush=True)


def run_fit(arm):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "fit", arm, str(ROUNDS)], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"fit arm {arm} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if SUB == "fit":
        return fit_arm(FIT_ARM)
    if SUB == "trace":
        from tf2_yolo_amd import images
        x = np.random.default_rng(1234).integers(0, 256, (32, HW, HW, 3), dtype=np.uint8)
        for _ in range(4):
            images.prepare(x, (HW, HW), rescale=S, resize=None)
        torch.cuda.synchronize()
        return
    both = SUB != "baseline"
    _, m = build()
    results = []
    for bs, calls in BATCHES:
        x = np.random.default_rng(1234).integers(0, 256, (bs, HW, HW, 3), dtype=np.uint8)
        arms = {
            "detect": (lambda: m.detect(host_f32(x), batch_size=bs, conf_threshold=THR),
                       lambda: m.detect_images(x, batch_size=bs, conf_threshold=THR, rescale=S)),
            "predict": (lambda: m.predict(host_f32(x), batch_size=bs), lambda: m.predict(x, batch_size=bs, rescale=S)),
        }
        for what, (fa, fb) in arms.items():
            a = listed(fa())
            rec = {"call": what, "batch": bs, "rounds": ROUNDS, "calls_per_run": calls}
            if what == "detect":
                rec["kept_per_image"] = sum(r.shape[0] for r in a) / bs
            if both:
                b = listed(fb())
                assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b)), (what, bs)
            for fn in (fa, fb) if both else (fa,):
                timed(fn, 2)
            ta, tb = [], []
            for _ in range(ROUNDS):
                ta.append(timed(fa, calls))
                if both:
                    tb.append(timed(fb, calls))
            rec["host_float32_ms"] = stats(ta)
            if both:
                rec["uint8_rescale_ms"] = stats(tb)
                rec["speedup"] = rec["host_float32_ms"]["median"] / rec["uint8_rescale_ms"]["median"]
                # slower = beyond the run-to-run spread of the two arms
                rec["uint8_slower"] = min(tb) > max(ta)
            print(json.dumps(rec), flush=True)
            results.append(rec)
    del m
    torch.cuda.empty_cache()
    fit = {"batch": FIT_BATCH, "batches": FIT_BATCHES, "host_float32": run_fit("A")}
    if both:
        fit["uint8_rescale"] = run_fit("B")
    print(json.dumps(fit), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "what": __doc__.split("usage")[0].strip(), "results": results, "fit": fit}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
