"""Golden vectors on grids with gh != gw, made by EXECUTING THE REFERENCE's own utils/tools.py and utils/measurement.py
(build container only; same stub modules as make_golden.py). Only outputs are stored (tests/golden/nonsquare_golden.npz);
the inputs are regenerated from the seeded functions of gen_inputs.py.

Run:  python -B tests/golden/make_nonsquare_golden.py

The file is written entry by entry with a fixed time stamp, so that a second run reproduces it byte for byte
(np.savez stamps every entry with the time of the run)."""
import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_inputs                      # noqa: E402
from make_golden import import_reference_tools   # noqa: E402

CLASS_NAMES = ["a", "b", "c"]


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    tools = import_reference_tools()
    from utils import measurement as M   # the reference's utils/measurement.py
    out = {}
    for key, C, thr, lv in gen_inputs.nonsquare_decode_cases():   # levels fine -> coarse
        dec = tools.decode(*lv, class_num=C, threshold=thr, version=3)
        assert dec.size and len(dec) > 20, "too few rows: pick another seed"
        out[f"{key}_decode"] = dec
        scores = dec[:, 4] * dec[:, 6]
        for c in range(C):   # ties only matter inside a class (argsort instability)
            sc = scores[dec[:, 5] == c]
            assert len(np.unique(sc)) == len(sc), "score tie: pick another seed"
        out[f"{key}_nms"] = tools.nms(dec, class_num=C, nms_threshold=0.5)
        out[f"{key}_diou"] = tools.nms(dec, class_num=C, nms_threshold=0.5, iou_mode=2)
        out[f"{key}_soft"] = tools.soft_nms(dec, class_num=C, nms_threshold=0.5, conf_threshold=thr, sigma=0.5)
        print(key, "rows", len(dec), "nms", len(out[f"{key}_nms"]), "diou", len(out[f"{key}_diou"]), "soft", len(out[f"{key}_soft"]))
    misc = gen_inputs.nonsquare_misc_inputs()
    out["v1_decode"] = tools.decode(misc["v1_lv"], class_num=4, threshold=0.4, version=1)
    out["v2_decode"] = tools.decode(misc["v2_lv"], class_num=20, threshold=0.8, version=2)
    lab = misc["label12x20"]
    l6 = tools.down2xlabel(lab)
    out["label6x10"] = l6
    out["label3x5"] = tools.down2xlabel(l6)
    out["label12x20_decode"] = tools.decode(lab[0], class_num=3, threshold=0.5, version=3)
    out["binary_weight"] = tools.get_class_weight(lab[..., 4:5], "binary")
    for m in ("alpha", "log", "effective"):
        out[f"class_weight_{m}"] = tools.get_class_weight(lab[..., 5:], m)
    # evaluation with labels on a 6 x 10 grid
    y_true, lv0, lv1 = gen_inputs.nonsquare_measurement_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = M.create_score_mat(y_true, lv0, lv1, class_names=CLASS_NAMES, version=3, **gen_inputs.NONSQUARE_SCORE_KW)
        for col in ("precision", "recall", "F1-score", "gts", "dets"):
            out[f"score_{col}"] = t[col].to_numpy()
        f = M.PRfunc(y_true, lv0, lv1, class_names=CLASS_NAMES, version=3, **gen_inputs.NONSQUARE_PR_KW)
        for c in range(len(CLASS_NAMES)):
            assert len(f.precisions[c]) > 3, "class with hardly any detection: pick another seed"
            out[f"pr_prec{c}"] = np.asarray(f.precisions[c], dtype=np.float64)
            out[f"pr_rec{c}"] = np.asarray(f.recalls[c], dtype=np.float64)
        for mode in ("voc2007", "voc2012", "area", "smootharea"):
            out[f"pr_map_{mode}"] = f.get_map(mode)["ap"].to_numpy().astype(np.float64)
    path = os.path.join(HERE, "nonsquare_golden.npz")
    save_npz(path, out)
    print("arrays:", len(out), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
