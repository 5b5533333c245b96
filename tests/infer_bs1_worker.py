"""BASELINE config 5's network as bench.py builds it (YOLOv3-416, 80 classes, synthetic_keras_weights seed 1234 with
residual_gamma 0.1, image rng(1234)): helpers for tests/test_gpu_infer_bs1.py, and a child process of that test.

The launch policy of csrc/conv_small.hip (YOLO_CONV_SMALL, YOLO_CONV_SMALL_TILE) is read once per process, so the test
runs its predict under those settings in a fresh process:
    python tests/infer_bs1_worker.py OUT.npy
writes the three outputs of Model.predict at bs 1 (coarse -> fine), flattened and concatenated, to OUT.npy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def c5_weights():
    from tf2_yolo_amd import graphs, labels
    return labels.synthetic_keras_weights(graphs.build_yolov3((416, 416, 3), 80), 1234, residual_gamma=0.1)


def c5_image():
    return np.random.default_rng(1234).random((1, 416, 416, 3), dtype=np.float32)


def set_weights(model, w):
    """w: synthetic_keras_weights of the model's graph; the anchor layers (YOLOv4) keep what create_model was given"""
    for n in model.layer_names():
        lay = model.get_layer(n)
        k = len(lay.get_weights())
        if k and not n.endswith("_anchor"):
            lay.set_weights([w[f"{n}/{i}"] for i in range(k)])


def build_c5(w):
    import yolov3
    y = yolov3.Yolo((416, 416, 3), [f"c{i}" for i in range(80)])
    y.create_model(pretrained_body=None)
    set_weights(y.model, w)
    return y.model


def main(out):
    pred = build_c5(c5_weights()).predict(c5_image(), batch_size=1)
    np.save(out, np.concatenate([p.ravel() for p in pred]))


if __name__ == "__main__":
    main(sys.argv[1])
