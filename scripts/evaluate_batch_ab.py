"""Validation mAP of a data set, before and after the evaluation moved to one device pipeline.
YOLOv3-416 (C = 80), synthetic weights (labels.synthetic_keras_weights, seed 1234, residual gamma 0.1), 256 rng(1234) images.
Labels and threshold come from the network's own predictions, so that there is something to match: the confidence
threshold is the one that leaves about 300 candidates per image, and on the (level, anchor) slice where most boxes pass it
every such cell is a ground truth with that box and its best class. Rows, each one call on the whole set (nms_mode 1, max_per_img 100):

  prfunc_host_arrays            PRfunc(y, *pred) + get_map() on predict's NumPy arrays
  score_mat_host_arrays         create_score_mat(y, *pred) on the same arrays
  predict_then_prfunc           Model.predict (every level to the host) + PRfunc + get_map()
  evaluate_detections           Model.evaluate_detections + prfunc() + get_map() + score_mat(): only where the tree has it

and the one-image / one-class entry points, which no row above calls, each one call on seeded rows:

  one_match_detections          ops.match_detections, 300 ground truths and 700 detections of 3 classes
  one_rank_desc                 ops.rank_desc, 3100 rows in seven segments
  one_pr_curve                  ops.pr_curve, 3100 rows and 300 ground truths, precision mode 2

"Before" is a second checkout (the parent commit, built) given with --before; "after" is the tree this script lies in. Every
measurement is a fresh process of one tree: one untimed call per row, then `calls` timed ones, host clock around synchronised
calls. The processes of the two trees alternate, `rounds` each, in one session on one box; the file keeps every sample, the
median and min / max per tree and row, and says where the two ranges overlap (a gain within the run-to-run spread). The
curves and tables of all rows and both trees must be equal, bit for bit, or nothing is written.

usage: evaluate_batch_ab.py --before DIR [--rounds 2] [--calls 3] [--images 256] [--out profiles/evaluate_batch_ab.json]
       evaluate_batch_ab.py child CALLS IMAGES          (one tree's measurement, JSON on the last line of stdout)"""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW, C = 416, 80
PER_IMAGE = 300
KW = dict(nms_mode=1, nms_threshold=0.5, iou_threshold=0.5)


def build():
    import yolov3
    from tf2_yolo_amd import graphs, labels
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


def labels_from(pred, np):
    tops = []
    for lv in pred:
        t = lv.reshape(*lv.shape[:3], 3, 5 + C)
        p = (t[..., 4:5] * t[..., 5:]).ravel()
        k = min(PER_IMAGE * len(lv), p.size)
        tops.append(np.partition(p, -k)[-k:])
    tops = np.concatenate(tops)
    k = PER_IMAGE * len(pred[0])
    thr = float(np.partition(tops, -k)[-k])
    best = (-1, None, None)
    for lv in pred:       # the (level, anchor) slice with the most boxes above the threshold carries the labels
        t = lv.reshape(*lv.shape[:3], 3, 5 + C)
        hits = (t[..., 4:5] * t[..., 5:]).max(axis=-1) >= thr
        a = int(hits.sum(axis=(0, 1, 2)).argmax())
        if int(hits[..., a].sum()) > best[0]:
            best = (int(hits[..., a].sum()), t[..., a, :].astype(np.float64), hits[..., a])
    _, t, hit = best
    y = t.copy()
    y[..., 4] = hit
    y[..., 5:] = np.eye(C)[t[..., 5:].argmax(axis=-1)] * hit[..., None]
    return y, thr


def digest(np, f, table=None):
    h = hashlib.sha256()
    for a in list(f.precisions) + list(f.recalls):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    if table is not None:
        for col in ("precision", "recall", "F1-score", "gts", "dets"):
            h.update(np.ascontiguousarray(table[col].to_numpy(), dtype=np.float64).tobytes())
    return h.hexdigest()


def child(calls, images):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tf2_yolo_amd import measurement
    assert torch.cuda.is_available(), "needs a GPU"
    names = [f"c{i}" for i in range(C)]
    m = build()
    x = np.random.default_rng(1234).random((images, HW, HW, 3), dtype=np.float32)
    pred = m.predict(x, batch_size=32)
    y, thr = labels_from(pred, np)
    kw = dict(conf_threshold=thr, **KW)
    seen = {}

    def prfunc_host():
        f = measurement.PRfunc(y, *pred, class_names=names, version=3, max_per_img=100, **kw)
        seen["map"] = float(f.get_map()["ap"].to_numpy()[-1])
        seen["curves"] = digest(np, f)

    def score_mat_host():
        t = measurement.create_score_mat(y, *pred, class_names=names, version=3, **kw)
        seen["table"] = hashlib.sha256(t.to_numpy().astype(np.float64).tobytes()).hexdigest()
        seen["gts"], seen["dets"] = int(t["gts"].sum()), int(t["dets"].sum())

    def predict_then_prfunc():
        p = m.predict(x, batch_size=32)
        f = measurement.PRfunc(y, *p, class_names=names, version=3, max_per_img=100, **kw)
        f.get_map()
        assert digest(np, f) == seen["curves"]

    def evaluate_detections():
        ev = m.evaluate_detections(x, y, names, batch_size=32, max_per_img=100, **kw)
        f = ev.prfunc()
        f.get_map()
        t = ev.score_mat()
        assert digest(np, f) == seen["curves"]
        assert hashlib.sha256(t.to_numpy().astype(np.float64).tobytes()).hexdigest() == seen["table"]

    from tf2_yolo_amd import ops
    rng = np.random.default_rng(4321)
    gt = np.concatenate((rng.random((300, 2)) * 0.8 + 0.1, rng.random((300, 2)) * 0.25 + 0.05, np.ones((300, 1)),
                         rng.integers(0, 3, (300, 1)), np.ones((300, 1))), axis=1)
    det = gt[rng.integers(0, 300, 700)]                   # noisy copies: several detections per ground truth
    det[:, :4] *= 1 + rng.normal(0, 0.05, (700, 4))
    det[:, 4], det[:, 6] = rng.random(700), rng.random(700)
    one = [rng.random(3100), rng.integers(0, 7, 3100).astype(np.int32), rng.integers(0, 300, 3100).astype(np.int32),
           (rng.random(3100) < 0.5).astype(np.uint8)]
    gt, det, key, seg, gid, hit = (torch.from_numpy(a).cuda() for a in [gt, det] + one)
    last = {}

    def one_match_detections():
        counts = torch.zeros((3, 4), device="cuda", dtype=torch.int64)
        last["one_match"] = ops.match_detections(gt, det, 3, 0.5, counts) + (counts,)

    def one_rank_desc():
        last["one_rank"] = (ops.rank_desc(key, seg),)

    def one_pr_curve():
        last["one_curve"] = ops.pr_curve(key, gid, hit, 300, 2)

    rows = [("prfunc_host_arrays", prfunc_host), ("score_mat_host_arrays", score_mat_host),
            ("predict_then_prfunc", predict_then_prfunc)]
    if hasattr(m, "evaluate_detections"):
        rows.append(("evaluate_detections", evaluate_detections))
    rows += [("one_match_detections", one_match_detections), ("one_rank_desc", one_rank_desc), ("one_pr_curve", one_pr_curve)]
    out = {}
    for name, fn in rows:
        fn()                                  # untimed: code objects, the caching allocator, the host buffers
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = ms
    for name, tensors in last.items():        # what the one-image / one-class calls gave: equal in both trees, like the curves
        seen[name] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in tensors)).hexdigest()
    print(json.dumps({"ms": out, "seen": seen, "conf_threshold": thr, "device": torch.cuda.get_device_name(0)}), flush=True)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": v}


def main():
    a = sys.argv[1:]
    if a and a[0] == "child":
        return child(int(a[1]), int(a[2]))
    opt = {"--rounds": "2", "--calls": "3", "--images": "256", "--out": os.path.join(ROOT, "profiles", "evaluate_batch_ab.json")}
    for k, v in zip(a[::2], a[1::2]):
        opt[k] = v
    before = os.path.abspath(opt["--before"])
    this = os.path.abspath(__file__)
    trees = {"before": os.path.join(before, "scripts", os.path.basename(this)), "after": this}
    if not os.path.exists(trees["before"]):       # the parent commit does not have this script: it runs this file's text
        raise SystemExit(f"copy {this} to {trees['before']} first")
    samples = {t: {} for t in trees}
    seen = {}
    for r in range(int(opt["--rounds"])):
        for tree, script in trees.items():
            p = subprocess.run([sys.executable, script, "child", opt["--calls"], opt["--images"]], cwd=os.path.dirname(os.path.dirname(script)),
                               stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"{tree} (round {r}) ended with status {p.returncode}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            print(tree, r, json.dumps(rec["ms"]), flush=True)
            for k, v in rec["ms"].items():
                samples[tree].setdefault(k, []).extend(v)
            if seen.setdefault("seen", rec["seen"]) != rec["seen"]:
                raise SystemExit(f"{tree} (round {r}) computed other curves or tables: {rec['seen']} != {seen['seen']}")
            seen["device"], seen["thr"] = rec["device"], rec["conf_threshold"]
    res = {t: {k: stats(v) for k, v in rows.items()} for t, rows in samples.items()}

    def compare(name, b, a_):
        lo, hi = (a_, b) if a_["median"] <= b["median"] else (b, a_)
        return {"row": name, "before_ms": b["median"], "after_ms": a_["median"], "speedup": b["median"] / a_["median"],
                "within_spread": lo["max"] >= hi["min"], "after_median_within_or_below_before_range": a_["median"] <= b["max"]}
    cmp_ = [compare(k, res["before"][k], res["after"][k]) for k in res["before"]]
    cmp_.append(compare("predict_then_prfunc (before) -> evaluate_detections (after)", res["before"]["predict_then_prfunc"],
                        res["after"]["evaluate_detections"]))
    out = {"device": seen["device"], "what": __doc__.split("usage")[0].strip(), "images": int(opt["--images"]), "classes": C,
           "conf_threshold": seen["thr"], "ground_truths": seen["seen"]["gts"], "detections_after_nms": seen["seen"]["dets"],
           "mAP_voc2012": seen["seen"]["map"], "rounds": int(opt["--rounds"]), "calls_per_round": int(opt["--calls"]),
           "results": res, "comparison": cmp_}
    os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
    with open(opt["--out"], "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(cmp_, indent=1))
    print("wrote", opt["--out"])


if __name__ == "__main__":
    main()
