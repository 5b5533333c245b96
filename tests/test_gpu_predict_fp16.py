"""Model.predict(x, precision="fp16") end to end: every planes convolution of the inference path on ONE fp16 MFMA pass
(csrc/planes.hpp), the stem and the convolutions without planes operands exact, on YOLOv3 (64 x 96, batch 1 and 3), YOLOv4
(160 x 96: Mish, the SPP concat, the head tile), tiny-YOLOv3 and YOLOv2 (64 x 64, batch 2: the pool path, space-to-depth,
biases), all with random weights.

Parity. The float64 oracle (oracle/models.py) runs twice: as it is, and with oracle.layers.conv2d wrapped so that x and w
are rounded to hx = fp16(s_x x) / s_x, hw = fp16(s_w w) / s_w (s = the power-of-two scale of the planes format from max|.|)
for exactly the convolutions with ops.planes_fwd_ok(cin, cout). With e_half = the distance of the two oracle runs and e_dev =
the distance of the device's fp16 predict from the plain oracle, both relative to each output's largest entry, the bar is
e_dev <= 1.5 e_half -- the margin test_gpu_infer_bs1._assert_parity gives the fp32 floor. The fp16 predict must also differ
from the fp32 one by more than min(1e-4, e_half / 3): the fp32 predict is within the fp32 floor of the oracle, the fp16 one
about e_half away from it."""
import gc
import math

import numpy as np
import pytest
import torch

import test_gpu_model as T
from oracle import layers as L
from test_gpu_model import _rel, log_parity_ratio

pytestmark = pytest.mark.gpu

# id -> (_setup arguments, images of the predict calls)
MODELS = {
    "v3-64x96": (dict(version=3, shape=(64, 96), N=3, class_num=2), (1, 3)),
    "v4-160x96": (dict(version=4, shape=(160, 96), N=1), (1,)),
    "tiny-v3-64": (dict(version=3, hw=64, N=2, tiny=True), (2,)),
    "v2-64": (dict(version=2, hw=64, N=2), (2,)),
}


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _scale_of(bound):
    """planes_scale_from_bound (csrc/planes.hpp): the power of two s with s * bound <= 2^15"""
    b = float(bound)
    if not b > 0:
        return 1.0
    return 2.0 ** (15 - math.frexp(b)[1])


def _rounded(t):
    s = _scale_of(t.abs().max())
    return (t * s).half().to(t.dtype) / s


def _oracle(fwd, w, x, half):
    """the float64 oracle's inference outputs; half: with the operands of the planes-capable convolutions fp16-rounded"""
    from tf2_yolo_amd import ops
    real = L.conv2d

    def conv2d_half(x, w_hwio, bias=None, stride=1, padding="same"):
        if ops.planes_fwd_ok(w_hwio.shape[2], w_hwio.shape[3]):
            x, w_hwio = _rounded(x), _rounded(w_hwio)
        return real(x, w_hwio, bias, stride=stride, padding=padding)
    w64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()}
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        if half:
            mp.setattr(L, "conv2d", conv2d_half)
        outs = fwd(w64, torch.tensor(x, dtype=torch.float64), False)[0]
    return [o.numpy() for o in outs]


def _setup(**kw):
    """test_gpu_model._setup (random kernels, biases, BatchNorm parameters and moving statistics) with the gamma of every unit
    in front of a residual Add x 0.1, config 5's recipe: in inference mode a random network doubles the variance at each Add
    (23 of them in Darknet-53), the heads' sigmoid / exp saturate to 0, 1 and inf, and saturated outputs compare nothing"""
    y, model, fwd, _, _, x, _ = T._setup(**kw)
    for u in model.net.units:
        if u.kind == "conv" and u.bn and u.residual is not None:
            lay = model.get_layer(u.name + "_bn")
            ws = lay.get_weights()
            ws[0] = ws[0] * 0.1
            lay.set_weights(ws)
    return y, model, fwd, x


def _listed(p):
    return p if isinstance(p, list) else [p]


@pytest.fixture(scope="module", params=list(MODELS))
def net_case(request):
    """model, images and the two oracle runs -- once per model"""
    import conftest
    conftest.foreground_threads()
    kw, batches = MODELS[request.param]
    y, model, fwd, x = _setup(**kw)
    w = T._weights_dict(model)
    case = {"id": request.param, "model": model, "fwd": fwd, "x": x, "batches": batches, "w": w,
            "o64": _oracle(fwd, w, x, False), "ohalf": _oracle(fwd, w, x, True)}
    assert all(np.isfinite(o).all() for o in case["o64"] + case["ohalf"])
    yield case
    del case["model"], model, y
    _free()


def _max_rel(a, b):
    return max(float(_rel(p, q)) for p, q in zip(a, b))


def test_predict_fp16_parity(net_case):
    m, x = net_case["model"], net_case["x"]
    for n in net_case["batches"]:
        xs = x[:n]
        o64, ohalf = [o[:n] for o in net_case["o64"]], [o[:n] for o in net_case["ohalf"]]
        p32 = _listed(m.predict(xs, batch_size=n))
        p32b = _listed(m.predict(xs, batch_size=n, precision="fp32"))
        p16 = _listed(m.predict(xs, batch_size=n, precision="fp16"))
        for a, b, c in zip(p32, p32b, p16):
            assert np.array_equal(a, b)                                  # default untouched
            assert a.shape == c.shape and np.isfinite(c).all() and not np.array_equal(a, c)
        e_half, e_dev, e32 = _max_rel(ohalf, o64), _max_rel(p16, o64), _max_rel(p32, o64)
        d_half, d32 = _max_rel(p16, ohalf), _max_rel(p16, p32)
        log_parity_ratio({"case": f"{net_case['id']} bs{n} predict fp16", "e_half": e_half, "fp16_err": e_dev,
                          "fp16_ratio": e_dev / max(e_half, 1e-30), "fp16_to_half_oracle": d_half, "fp16_to_fp32_predict": d32,
                          "forward_err": e32})
        assert e_dev <= 1.5 * e_half, (net_case["id"], n, e_dev, e_half)
        assert d32 > min(1e-4, e_half / 3), (net_case["id"], n, d32, e_half)
        assert e32 < max(1e-4, e_half / 3), (net_case["id"], n, e32)      # (the fp32 predict is not what moved)


def test_graph_cache_keeps_the_precisions_apart(net_case):
    """fp16, fp32, fp16 again, then a second image: each precision bit-identical to its own first result and to the eager
    Network.forward of that precision; one captured graph per (batch size, precision), none captured twice"""
    m, x = net_case["model"], net_case["x"]
    net = m.net
    if not net._use_infer_graph:
        pytest.fail("the inference graph is switched off in this environment")
    net.mark_params_changed()
    x1 = torch.from_numpy(x[:1]).cuda()
    x2 = torch.from_numpy(np.random.default_rng(5).random(x[:1].shape, dtype=np.float32)).cuda()
    clone = lambda outs: [o.clone() for o in outs]
    a16 = clone(net.infer(x1, precision="fp16"))
    g16 = net._infer_graphs[(1, "fp16")][0]
    a32 = clone(net.infer(x1, precision="fp32"))
    g32 = net._infer_graphs[1][0]
    b16 = clone(net.infer(x1, precision="fp16"))
    b32 = clone(net.infer(x1))
    c16 = clone(net.infer(x2, precision="fp16"))
    c32 = clone(net.infer(x2, precision="fp32"))
    d16 = clone(net.infer(x1, precision="fp16"))
    assert set(net._infer_graphs) == {1, (1, "fp16")}
    assert net._infer_graphs[(1, "fp16")][0] is g16 and net._infer_graphs[1][0] is g32      # no re-capture
    e16_1 = clone(net.forward(x1, training=False, precision="fp16"))
    e32_1 = clone(net.forward(x1, training=False))
    e16_2 = clone(net.forward(x2, training=False, precision="fp16"))
    e32_2 = clone(net.forward(x2, training=False, precision="fp32"))
    torch.cuda.synchronize()
    for i in range(len(a16)):
        assert torch.equal(a16[i], b16[i]) and torch.equal(a16[i], d16[i]) and torch.equal(a16[i], e16_1[i])
        assert torch.equal(a32[i], b32[i]) and torch.equal(a32[i], e32_1[i])
        assert torch.equal(c16[i], e16_2[i]) and torch.equal(c32[i], e32_2[i])
        assert not torch.equal(a16[i], a32[i]) and not torch.equal(c16[i], c32[i])          # no cross-talk
        assert not torch.equal(a16[i], c16[i]) and not torch.equal(a32[i], c32[i])          # the second image is another one


def test_weight_changes_reach_both_precisions():
    """set_weights (one unit's gamma x 3, another's moving variance / 4) drops the graphs of both precisions; both predicts
    then hold the new network: fp32 within the fp32 floor's bar of the new float64 oracle; fp16 -- a stale graph, filter
    plane or folded scale would leave it `moved` away from the new oracle, `moved` = how far the change took the outputs --
    within a quarter of `moved`, fp16 operand rounding (e_half, from the two oracle runs) being a tenth of it at most"""
    y, model, fwd, x = _setup(version=3, shape=(64, 96), N=1, class_num=2)
    old16 = _listed(model.predict(x, batch_size=1, precision="fp16"))
    old32 = _listed(model.predict(x, batch_size=1))
    assert set(model.net._infer_graphs) == {1, (1, "fp16")}
    bns = [u.name + "_bn" for u in model.net.units if u.kind == "conv" and u.bn and u.residual is None]
    for name, idx, f in ((bns[2], 0, 3.0), (bns[4], 3, 0.25)):
        lay = model.get_layer(name)
        ws = lay.get_weights()
        ws[idx] = ws[idx] * f
        lay.set_weights(ws)
    assert not model.net._infer_graphs
    w = T._weights_dict(model)
    o64, ohalf = _oracle(fwd, w, x, False), _oracle(fwd, w, x, True)
    with torch.no_grad():
        o32 = [o.numpy() for o in fwd({k: torch.tensor(v, dtype=torch.float32) for k, v in w.items()},
                                      torch.tensor(x, dtype=torch.float32), False)[0]]
    floor, e_half = _max_rel(o32, o64), _max_rel(ohalf, o64)
    new16 = _listed(model.predict(x, batch_size=1, precision="fp16"))
    new32 = _listed(model.predict(x, batch_size=1))
    assert all(np.isfinite(o).all() for o in o64 + old32)
    moved = min(float(_rel(a, b)) for a, b in zip(old32, o64))
    e32, e16 = _max_rel(new32, o64), _max_rel(new16, o64)
    print(f"after set_weights: outputs moved {moved:.3g}; fp32 {e32:.3g} (floor {floor:.3g}), fp16 {e16:.3g} (e_half {e_half:.3g})")
    assert moved > 1e-3 and e_half < 0.1 * moved                               # the change moves every output, far more than fp16
    assert e32 < max(1e-4, 1.5 * floor)
    assert e16 < 0.25 * moved
    for a, b in zip(old16, new16):
        assert not np.array_equal(a, b)
    del y, model
    _free()


def test_argument_validation():
    from tf2_yolo_amd import _lib
    y, model, fwd, x = _setup(version=3, tiny=True, hw=64, N=1)
    with pytest.raises(ValueError, match="precision"):
        model.predict(x, precision="int8")
    with pytest.raises(ValueError, match="precision"):
        model.net.infer(torch.from_numpy(x).cuda(), precision="half")
    with pytest.raises(ValueError):
        model.net.forward(torch.from_numpy(x).cuda(), training=True, precision="fp16")
    assert not model.net.training and not model.net._infer_graphs           # nothing ran
    # a training forward and backward-capable state are unaffected by an earlier fp16 inference
    model.predict(x, precision="fp16")
    outs = model.net.forward(torch.from_numpy(x).cuda(), training=True)
    torch.cuda.synchronize()
    assert model.net._precision == "fp32" and all(bool(torch.isfinite(o).all()) for o in outs)
    del y, model
    _free()
