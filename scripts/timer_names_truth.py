"""Are the kernel names of ops.KernelTimer true? One eager YOLOv3-416 training step (batch 4) with the timer on from the
start of the process, under a kernel trace; then the traced launches, summed per family, beside the timer's own table.

    rocprofv3 --kernel-trace --stats -d OUT/prof -o step --output-format csv -- python scripts/timer_names_truth.py step OUT
    python scripts/timer_names_truth.py compare OUT        # prints the table as JSON; exit status 1 if a family differs

The trace names carry every template argument, the timer's the leading ones: family() below is the mapping that bench.py
documents in hbm_traffic_from_profile. Reduce kernels, bias sums and planes passes belong to no family."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def family(trace_name):
    m = re.match(r"(?:void )?yolo::(\w+)(?:<([^>]*)>)?", trace_name)
    if m is None:
        return None
    base, a = m.group(1), [s.strip() for s in (m.group(2) or "").split(",")]
    if base in ("gather_conv_planes_kernel", "gather_conv_split_kernel", "wgrad_planes_kernel", "wgrad_split_kernel"):
        return f"{base}<{','.join(a[:4])}>"
    if base == "conv_win_kernel":     # <WGM, window chunks, stamps, split, stream-K, WGN, GEO, ...>: GEO = 1 is the patch form
        return f"conv_patch_planes_kernel<{64 * int(a[0])},{64 * int(a[5])}>" if int(a[6]) else f"conv_win_planes_kernel<{64 * int(a[0])},128>"
    if base in ("wgrad_win_kernel", "wgrad_win2_kernel", "wgrad_win16_kernel"):
        return "wgrad_win_planes_kernel<128,288%s>" % (",mfma16" if base == "wgrad_win16_kernel" else "")
    if base == "gather_conv_kernel":
        return f"{base}<{a[0]},{a[1]}{',flat' if a[4] == 'true' else ''}>"
    if base == "conv_small_kernel":
        return f"conv_small_planes_kernel<{32 * int(a[1])},{32 * int(a[2])}>"
    if base in ("stem_mfma_kernel", "stem_conv3x3_kernel"):
        return "stem_conv3x3_kernel"
    return base if base in ("wgrad_kernel", "stem_bn_bwd_wgrad_kernel") else None


def step(out):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from tf2_yolo_amd import ops
    ops.create_side_streams()
    import yolov3
    from tf2_yolo_amd import labels, optimizers
    ops.TIMER = timer = ops.KernelTimer()     # before the first launch of the process: the trace sees every launch, so must the timer
    yolo = yolov3.Yolo((416, 416, 3), [f"c{i}" for i in range(80)])
    yolo.create_model(pretrained_body=None, seed=1234)
    yolo.model.compile(optimizer=optimizers.Adam(learning_rate=1e-4), loss=yolo.loss())
    x, ys = labels.synthetic_batch(np.random.default_rng(1234), 4, (416, 416), 80)
    yolo.model.train_step_device(torch.from_numpy(x).cuda(), [torch.from_numpy(y).cuda() for y in ys])
    ops.TIMER = None
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "timer.json"), "w") as f:
        json.dump({k: v["launches"] for k, v in timer.summary().items()}, f, indent=1, sort_keys=True)


def compare(out):
    timer = json.load(open(os.path.join(out, "timer.json")))
    traced = {}
    for row in csv.DictReader(open(os.path.join(out, "prof", "step_kernel_stats.csv"))):
        fam = family(row["Name"])
        if fam is not None:
            traced[fam] = traced.get(fam, 0) + int(row["Calls"])
    table = {k: {"timer_launches": timer.get(k, 0), "traced_launches": traced.get(k, 0)} for k in sorted(set(timer) | set(traced))}
    print(json.dumps(table, indent=1))
    return int(any(v["timer_launches"] != v["traced_launches"] for v in table.values()))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("step", "compare"):
        sys.exit(__doc__)
    sys.exit(step(sys.argv[2]) if sys.argv[1] == "step" else compare(sys.argv[2]))
