"""CPU-only checks of the backbone classifiers: constructor argument handling, the symbolic graphs (parameter counts, trunk
unit names) and tests/classifier_ref.py, the float64 statement of the top that the GPU tests compare against, checked here
against torch float64 autograd."""
import inspect

import numpy as np
import pytest
import torch

import classifier_ref as R

from tf2_yolo_amd import bodies, engine, graphs


# ---- constructors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctor", [bodies.darknet53, bodies.csp_darknet53], ids=["darknet53", "csp_darknet53"])
def test_imagenet_weights_need_a_download_and_keep_the_reference_checks(ctor):
    with pytest.raises(ValueError, match="download"):
        ctor()                                           # defaults: include_top=True, weights="imagenet", 448, 1000 classes
    with pytest.raises(ValueError, match="download"):
        ctor(include_top=False)
    with pytest.raises(ValueError, match="`class_num` should be 1000"):
        ctor(weights="imagenet", class_num=10)
    with pytest.raises(ValueError, match=r"\(32x, 32x, 3\)"):
        ctor(weights="imagenet", input_shape=(100, 96, 3))


def test_exports():
    import yolov1_5.models
    import yolov3.models
    import yolov4.models
    assert yolov1_5.models.darknet is bodies.darknet
    assert yolov3.models.darknet53 is bodies.darknet53
    assert yolov4.models.csp_darknet53 is bodies.csp_darknet53
    import yolov2.models
    assert yolov2.models.darknet19 is bodies.darknet19
    assert list(inspect.signature(bodies.darknet19).parameters)[:2] == ["input_shape", "class_num"]
    assert list(inspect.signature(bodies.darknet).parameters)[:2] == ["input_shape", "class_num"]
    for f in (bodies.darknet53, bodies.csp_darknet53):
        assert list(inspect.signature(f).parameters)[:4] == ["include_top", "weights", "input_shape", "class_num"]
        assert inspect.signature(f).parameters["weights"].default == "imagenet"


# ---- symbolic graphs ------------------------------------------------------------------------------------------------------
GRAPHS = {
    "darknet": (graphs.build_darknet, lambda s: graphs.yolov1_5_body(s)[0], (256, 256, 3)),
    "darknet53": (graphs.build_darknet53, lambda s: graphs.yolov3_body(s)[0], (256, 256, 3)),
    "csp_darknet53": (graphs.build_csp_darknet53, lambda s: graphs.yolov4_body(s)[0], (256, 256, 3)),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graph_is_the_detector_trunk_plus_the_top(name):
    build, body, shape = GRAPHS[name]
    K = 7
    clf, trunk, det = build(shape, K), build(shape, K, include_top=False), body(shape)
    n_trunk = len(trunk.units)
    # the trunk's units are exactly the first units of the detector's body, names and kinds
    assert [(u.name, u.kind) for u in trunk.units] == [(u.name, u.kind) for u in det.units[:n_trunk]]
    assert [u.name for u in clf.units] == [u.name for u in trunk.units] + ["top_gap", "top_dense"]
    C = trunk.units[-1].out.c
    assert C == 1024
    t0, s0 = engine.count_params(trunk)
    assert engine.count_params(clf) == (t0 + C * K + K, s0)
    # one output each: [N, K] probabilities / the feature map
    assert [o.shape for o in clf.outputs] == [(None, K)]
    assert [o.shape for o in trunk.outputs] == [(None, shape[0] // (64 if name == "darknet" else 32),
                                                shape[1] // (64 if name == "darknet" else 32), C)]


def test_darknet19_graph():
    """the Darknet-19 trunk of yolov2's body, then the class convolution with its BatchNorm, the pooling and a softmax"""
    K = 10
    clf, det = graphs.build_darknet19((416, 416, 3), K), graphs.yolov2_body((416, 416, 3))[0]
    names = [u.name for u in clf.units]
    assert names[-3:] == ["top", "top_gap", "top_softmax"] and [u.kind for u in clf.units[-3:]] == ["conv", "gap", "softmax"]
    n_trunk = len(names) - 3
    assert names[:n_trunk] == [u.name for u in det.units[:n_trunk]] and names[n_trunk - 1] == "conv6_5"
    trunk = engine.GraphBuilder((416, 416, 3))
    graphs.darknet19_body(trunk, trunk.input)
    t0, s0 = engine.count_params(trunk)
    assert engine.count_params(clf) == (t0 + 1024 * K + K + 2 * K, s0 + 2 * K)      # kernel, bias, gamma, beta; moving stats
    assert [o.shape for o in clf.outputs] == [(None, K)]
    top = clf.units[-3]
    assert (top.k, top.cout, top.bias, top.bn, (top.out.h, top.out.w)) == (1, K, True, True, (13, 13))


def test_plan_of_a_classifier_graph():
    """the gap unit reads the fp32 form of the last activation; everything in front of the Dense layer needs a gradient"""
    from tf2_yolo_amd import plan
    b = graphs.build_darknet53((64, 64, 3), 5)
    g = plan.plan_graph(b.units, b.tensors, b.input, b.outputs, plan.Options.from_env({}))
    last = b.units[-3]
    assert last.kind == "conv" and last.a_needed
    assert g.needs_grad[b.units[-1].out.tid] and g.needs_grad[b.units[-2].out.tid]
    assert [plan.has_params(u) for u in b.units[-3:]] == [True, False, True]


def test_dense_needs_a_pooled_tensor():
    b = engine.GraphBuilder((32, 32, 3))
    x = b.conv(b.input, 32, 3, "c")
    with pytest.raises(ValueError, match="gap"):
        b.dense_softmax(x, 3, "d")


# ---- classifier_ref against torch float64 autograd --------------------------------------------------------------------------
def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


@pytest.mark.parametrize("shape", R.GAP_CASES)
def test_ref_gap(shape):
    rng = np.random.default_rng(1)
    N, H, W, C = shape
    x, dg = rng.standard_normal(shape), rng.standard_normal((N, C))
    xt = _t(x, True)
    gt = xt.mean(dim=(1, 2))
    gt.backward(_t(dg))
    np.testing.assert_allclose(R.gap_fwd(x), gt.detach().numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(R.gap_bwd(dg, H, W), xt.grad.numpy(), rtol=0, atol=1e-13)


@pytest.mark.parametrize("case", R.DENSE_CASES + R.SOFTMAX_CASES)
def test_ref_dense_softmax(case):
    rng = np.random.default_rng(2)
    N, C, K = case
    null = case in R.SOFTMAX_CASES
    g, dp = rng.standard_normal((N, C)), rng.standard_normal((N, K))
    W = None if null else rng.standard_normal((K, C)) * (60.0 / np.sqrt(C))      # logits spread over tens
    b = None if null else rng.standard_normal(K)
    gt = _t(g, True)
    Wt, bt = (None, None) if null else (_t(W, True), _t(b, True))
    zt = gt if null else gt @ Wt.T + bt
    pt = torch.softmax(zt, dim=1)
    pt.backward(_t(dp))
    z, p = R.dense_softmax_fwd(g, W, b)
    dz, dg, dW, db = R.dense_softmax_bwd(dp, p, g, W)
    np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dg, gt.grad.numpy(), rtol=1e-9, atol=1e-12)
    if not null:
        np.testing.assert_allclose(dW, Wt.grad.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("case", R.DENSE_CASES + R.SOFTMAX_CASES)
def test_ref_cce_and_accuracy(case):
    rng = np.random.default_rng(3)
    N, _, K = case
    p = R.softmax(rng.standard_normal((N, K)) * 2) * rng.uniform(0.5, 1.5, (N, 1))    # rows need not sum to 1
    t = R.one_hot(rng.integers(0, K, N), K)
    t[0] = R.softmax(rng.standard_normal((1, K)))[0]                                    # a soft-label row
    pt = _t(p, True)
    q = pt / pt.sum(dim=1, keepdim=True)
    loss = (-(_t(t) * torch.log(torch.clamp(q, R.EPS, 1 - R.EPS))).sum(dim=1)).mean()
    (loss * 3.0).backward()
    assert abs(R.cce(t, p) - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    np.testing.assert_allclose(R.cce_grad(t, p, grad_scale=3.0), pt.grad.numpy(), rtol=1e-9, atol=1e-12)
    want = (torch.argmax(_t(t), dim=1) == torch.argmax(pt.detach(), dim=1)).double().mean().item()
    assert R.accuracy(t, p) == want


def test_ref_cce_clip_passes_no_gradient_outside_its_range():
    p = np.array([[1e-9, 1 - 1e-9], [0.25, 0.75]])
    t = np.array([[1.0, 0.0], [1.0, 0.0]])
    d = R.cce_grad(t, p)
    assert (d[0] == 0).all() and (d[1] != 0).all()
    assert abs(R.cce(t, p) - 0.5 * (-np.log(1e-7) - np.log(0.25))) < 1e-12
    pt = _t(p, True)
    q = pt / pt.sum(dim=1, keepdim=True)
    (-(_t(t) * torch.log(torch.clamp(q, R.EPS, 1 - R.EPS))).sum(dim=1)).mean().backward()
    np.testing.assert_allclose(d, pt.grad.numpy(), rtol=1e-9, atol=0)


def test_ref_accuracy_ties_go_to_the_lowest_index():
    t = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    p = np.array([[0.2, 0.4, 0.4], [0.4, 0.2, 0.4]])
    assert R.accuracy(t, p) == 1.0
    assert R.accuracy(t[:, ::-1], p[:, ::-1]) == 0.0


@pytest.mark.parametrize("P,C", R.BN_CASES)
def test_ref_batchnorm_leaky(P, C):
    rng = np.random.default_rng(4)
    y, dout = rng.standard_normal((P, C)) * 2 + 0.3, rng.standard_normal((P, C))
    gamma, beta = 1 + 0.2 * rng.standard_normal(C), 0.1 * rng.standard_normal(C)
    yt, gt, bt = _t(y, True), _t(gamma, True), _t(beta, True)
    mean, var = yt.mean(dim=0), yt.var(dim=0, unbiased=False)
    out = torch.nn.functional.leaky_relu(gt * (yt - mean) / torch.sqrt(var + R.BN_EPS) + bt, 0.1)
    out.backward(_t(dout))
    got, m, v, _ = R.bn_leaky_fwd(y, gamma, beta)
    dy, dgamma, dbeta = R.bn_leaky_bwd(y, dout, gamma, beta)
    np.testing.assert_allclose(got, out.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dy, yt.grad.numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(dgamma, gt.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dbeta, bt.grad.numpy(), rtol=1e-9, atol=1e-11)
    mm, mv = R.bn_moving(np.zeros(C), np.ones(C), m, v, P, True, offset=0.5)
    np.testing.assert_allclose(mm, 0.01 * (m + 0.5), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mv, 0.99 + 0.01 * (v * P / (P - 1) if P > 1 else v), rtol=1e-12)
