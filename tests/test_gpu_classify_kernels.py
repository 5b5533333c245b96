"""The kernels of csrc/classify.hip against tests/classifier_ref.py (float64 NumPy, itself checked against torch autograd in
tests/test_classifier_cpu.py). Bar: 1e-4 of the largest entry of the compared tensor, the project's fp32 bar. Every kernel is
also run twice on the same inputs: no atomics, one summation order, so the two results are bit-equal."""
import numpy as np
import pytest
import torch

import classifier_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def f32(a):
    """the float32 values the device sees, as float64 for the reference"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def close(got, want, what, rounding=0.0):
    """rounding: an absolute allowance for float32 roundings that are not the kernel's arithmetic (stated where it is used)"""
    got, want = got.detach().cpu().numpy().astype(np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{what}: max error {err:.3e}, largest entry {scale:.3e}")
    assert err <= TOL * max(scale, 1e-30) + rounding, what


@pytest.mark.parametrize("shape", R.GAP_CASES)
def test_gap_forward_backward(shape):
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(10)
    N, H, W, C = shape
    x, dg, base = f32(rng.standard_normal(shape) + 0.5), f32(rng.standard_normal((N, C))), f32(rng.standard_normal(shape))
    g1, g2 = ops.gap_fwd(dev(x)), ops.gap_fwd(dev(x))
    close(g1, R.gap_fwd(x), "gap forward")
    assert torch.equal(g1, g2)
    want = R.gap_bwd(dg, H, W)
    for accumulate in (False, True):
        outs = []
        for _ in range(2):
            dx = dev(base) if accumulate else torch.full(shape, float("nan"), device="cuda")
            ops.gap_bwd(dev(dg), dx, accumulate=accumulate)
            outs.append(dx)
        close(outs[0], base + want if accumulate else want, f"gap backward accumulate={accumulate}")
        assert torch.equal(outs[0], outs[1])


def _dense_inputs(case, spread=None):
    rng = np.random.default_rng(11)
    N, C, K = case
    g = f32(np.abs(rng.standard_normal((N, C))))            # pooled LeakyReLU / Mish activations
    W = f32(rng.standard_normal((K, C)) / np.sqrt(C))
    b = f32(rng.standard_normal(K) * 0.1)
    if spread is not None:                                  # logits spread over +-spread
        z = g @ W.T
        W = f32(W * (spread / np.abs(z).max()))
        b = f32(np.zeros(K))
    dp = f32(rng.standard_normal((N, K)))
    return g, W, b, dp


@pytest.mark.parametrize("case,spread", [(c, None) for c in R.DENSE_CASES] + [((3, 96, 65), 60.0)])
def test_dense_softmax_forward_backward(case, spread):
    from tf2_yolo_amd import ops
    N, C, K = case
    g, W, b, dp = _dense_inputs(case, spread)
    z_ref, p_ref = R.dense_softmax_fwd(g, W, b)
    if spread is not None:
        assert np.abs(z_ref).max() > 0.99 * spread and z_ref.max() > 0.5 * spread and z_ref.min() < -0.5 * spread
        assert np.isfinite(p_ref).all()
    runs = []
    for _ in range(2):
        z, p = ops.dense_softmax_fwd(dev(g), dev(W), dev(b))
        runs.append((z, p))
    close(runs[0][0], z_ref, "logits")
    close(runs[0][1], p_ref, "probabilities")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # backward from the device's own probabilities (float32), dW / db as increments onto a non-zero buffer
    p = runs[0][1]
    p64 = p.cpu().numpy().astype(np.float64)
    _, dg_ref, dW_ref, db_ref = R.dense_softmax_bwd(dp, p64, g, W)
    rng = np.random.default_rng(12)
    dW0, db0 = f32(rng.standard_normal((K, C))), f32(rng.standard_normal(K))
    outs = []
    for _ in range(2):
        dg = torch.full((N, C), float("nan"), device="cuda")
        dW, db = dev(dW0), dev(db0)
        ops.dense_softmax_bwd(dev(dp), p, dev(g), dev(W), dg, dw=dW, db=db)
        outs.append((dg, dW, db))
    close(outs[0][0], dg_ref, "dg")
    close(outs[0][1], dW0 + dW_ref, "dW")
    close(outs[0][2], db0 + db_ref, "db")
    # the increments themselves: `buffer += increment` rounds the SUM to float32, half an ulp of the buffer's largest entry,
    # whatever the increment's size; the subtraction below is exact (Sterbenz) or rounds once more
    ulp = lambda a: 2.0 ** -23 * np.abs(a).max()      # noqa: E731
    close(outs[0][1] - dev(dW0), dW_ref, "dW increment", rounding=ulp(dW0 + dW_ref))
    close(outs[0][2] - dev(db0), db_ref, "db increment", rounding=ulp(db0 + db_ref))
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(a, c)


@pytest.mark.parametrize("case", R.SOFTMAX_CASES)
def test_softmax_without_weights(case):
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(13)
    N, C, K = case
    g, dp = f32(rng.standard_normal((N, C)) * 3), f32(rng.standard_normal((N, K)))
    gd = dev(g)
    (z, p), (_, p2) = ops.dense_softmax_fwd(gd, None, None), ops.dense_softmax_fwd(gd, None, None)
    assert z is gd and torch.equal(p, p2)
    close(p, R.dense_softmax_fwd(g)[1], "softmax")
    _, dg_ref, _, _ = R.dense_softmax_bwd(dp, p.cpu().numpy().astype(np.float64), g)
    dg, dg2 = torch.empty((N, K), device="cuda"), torch.empty((N, K), device="cuda")
    ops.dense_softmax_bwd(dev(dp), p, None, None, dg)
    ops.dense_softmax_bwd(dev(dp), p, None, None, dg2)
    close(dg, dg_ref, "dg = dz")
    assert torch.equal(dg, dg2)


def _cce_inputs(N, K, seed=14):
    """p rows from a softmax with every entry in [1e-5, 1 - 1e-5]; t one-hot plus one soft-label row"""
    rng = np.random.default_rng(seed)
    p = f32(R.softmax(rng.standard_normal((N, K)) * 0.8))
    assert p.min() >= 1e-5 and p.max() <= 1 - 1e-5
    t = R.one_hot(rng.integers(0, K, N), K)
    t[N - 1] = R.softmax(rng.standard_normal((1, K)))[0]
    return f32(t), p


@pytest.mark.parametrize("N,K", [(1, 2), (5, 3), (3, 65), (32, 1000), (37, 10)])
def test_cross_entropy_value_and_gradient(N, K):
    from tf2_yolo_amd import ops
    t, p = _cce_inputs(N, K)
    runs = [ops.cce_fwd_bwd(dev(t), dev(p), grad_scale=0.5) for _ in range(2)]
    loss, dpred = runs[0]
    want = R.cce(t, p)
    got = float(loss[0].item())
    print(f"loss {got!r} reference {want!r}")
    assert abs(got - want) <= TOL * abs(want)
    assert (loss[1:] == 0).all()
    close(dpred, R.cce_grad(t, p, grad_scale=0.5), "dpred")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the loss object: value alone, and value + gradient into given buffers
    from tf2_yolo_amd.losses import CategoricalCrossentropy
    L = CategoricalCrossentropy()
    assert abs(float(L(t, p).item()) - want) <= TOL * abs(want)
    buf, d = torch.zeros(8, device="cuda", dtype=torch.float64), torch.empty((N, K), device="cuda")
    L.fwd_bwd(dev(t), dev(p), grad_scale=1.0, dpred=d, loss_out=buf)
    close(d, R.cce_grad(t, p), "dpred through the loss object")
    assert float(buf[0].item()) == got


def test_cross_entropy_clipped_true_class():
    """a true-class probability of 1e-9: the value is -log(1e-7) for that row, and the clip passes no gradient"""
    from tf2_yolo_amd import ops
    t, p = _cce_inputs(4, 5)
    t[1] = [0, 0, 1, 0, 0]
    p[1] = f32([0.25, 0.25, 1e-9, 0.25, 0.25 - 1e-9])
    loss, dpred = ops.cce_fwd_bwd(dev(t), dev(p))
    want = R.cce(t, p)
    assert abs(float(loss[0].item()) - want) <= TOL * abs(want)
    assert float(dpred[1, 2].item()) == 0.0


def test_categorical_accuracy():
    from tf2_yolo_amd import ops
    from tf2_yolo_amd.losses import CategoricalAccuracy
    rng = np.random.default_rng(15)
    for N, K in [(1, 2), (7, 3), (33, 65), (32, 1000)]:
        p = f32(R.softmax(rng.standard_normal((N, K)) * 4))
        t = f32(R.one_hot(rng.integers(0, K, N), K))
        t[: N // 2] = f32(R.one_hot(np.argmax(p[: N // 2], axis=1), K))     # half of the rows are hits
        # rows whose two largest entries are closer than 1e-3 are redrawn from a sharper softmax: none is left out
        for i in np.nonzero(R.top_gap(p) <= 1e-3)[0]:
            p[i] = f32(R.one_hot([i % K], K)[0] * 0.9 + 0.1 / K)
        assert (R.top_gap(p) > 1e-3).all() and (R.top_gap(t) > 1e-3).all()
        a1, a2 = ops.categorical_accuracy(dev(t), dev(p)), ops.categorical_accuracy(dev(t), dev(p))
        assert float(a1[0].item()) == R.accuracy(t, p)
        assert torch.equal(a1, a2)
        assert float(CategoricalAccuracy()(t, p).item()) == pytest.approx(R.accuracy(t, p), abs=1e-7)


def test_categorical_accuracy_tie_goes_to_the_lowest_index():
    from tf2_yolo_amd import ops
    K = 130                      # ties across lanes and across a lane's own elements (k, k + 64, k + 128)
    p = np.full((4, K), 0.001, dtype=np.float32)
    p[0, [3, 67]] = 0.4          # same lane: 3 wins
    p[1, [70, 5]] = 0.4          # different lanes: 5 wins
    p[2, [129, 64]] = 0.4        # 64 wins
    p[3, :] = 0.25               # all equal: 0 wins
    for rows, want in (([3, 5, 64, 0], 1.0), ([67, 70, 129, 1], 0.0), ([3, 70, 64, 1], 0.5)):
        t = R.one_hot(rows, K)
        assert R.accuracy(t, p) == want
        assert float(ops.categorical_accuracy(dev(t), dev(p))[0].item()) == want


def test_size_checks():
    from tf2_yolo_amd import ops
    from tf2_yolo_amd._lib import YoloHipError
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    with pytest.raises(YoloHipError):
        ops.gap_fwd(z(2, 3, 3, 8), out=z(2, 4))
    with pytest.raises(YoloHipError):
        ops.gap_bwd(z(2, 4), z(2, 3, 3, 8))
    with pytest.raises(YoloHipError):
        ops.dense_softmax_fwd(z(2, 8), z(3, 7), z(3))
    with pytest.raises(YoloHipError):
        ops.dense_softmax_fwd(z(2, 8), z(3, 8), None)
    with pytest.raises(YoloHipError):
        ops.dense_softmax_bwd(z(2, 3), z(2, 3), z(2, 8), z(3, 8), z(2, 8), dw=z(3, 8), db=z(4))
    with pytest.raises(YoloHipError):
        ops.cce_fwd_bwd(z(2, 3), z(2, 4))
    with pytest.raises(YoloHipError):
        ops.categorical_accuracy(z(2, 3), z(3, 3))


@pytest.mark.parametrize("P,C", R.BN_CASES)
def test_batchnorm_over_any_channel_count(P, C):
    """yolo_bn_act_any_fwd / _bwd (darknet19's class convolution: class_num channels) against classifier_ref; the inputs keep
    every pre-activation at least 1e-3 from the LeakyReLU kink, asserted, so both executions take the same branches"""
    from tf2_yolo_amd import ops
    from tf2_yolo_amd._lib import ACT_LEAKY
    rng = np.random.default_rng(16)
    y, dout = f32(rng.standard_normal((P, C)) * 2 + 0.3), f32(rng.standard_normal((P, C)))
    gamma, beta, bias = f32(1 + 0.2 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C)), f32(rng.standard_normal(C))
    mm0, mv0 = f32(0.1 * rng.standard_normal(C)), f32(0.5 + rng.random(C))
    out_ref, mean, var, xhat = R.bn_leaky_fwd(y, gamma, beta)
    z = gamma * xhat + beta
    for i in np.argwhere(np.abs(z) < 1e-3):          # move the few near the kink away from it (and recompute)
        y[tuple(i)] = f32(y[tuple(i)] + 0.05)
    out_ref, mean, var, xhat = R.bn_leaky_fwd(y, gamma, beta)
    assert (np.abs(gamma * xhat + beta) >= 1e-4).all()
    dy_ref, dgamma_ref, dbeta_ref = R.bn_leaky_bwd(y, dout, gamma, beta)
    mm_ref, mv_ref = R.bn_moving(mm0, mv0, mean, var, P, True, offset=bias)
    z4 = lambda: torch.zeros(C, device="cuda")      # noqa: E731
    runs = []
    for _ in range(2):
        mm, mv, scale, shift, smean, sinv, out = dev(mm0), dev(mv0), z4(), z4(), z4(), z4(), torch.empty((P, C), device="cuda")
        ops.bn_act_any_fwd(dev(y), C, dev(gamma), dev(beta), mm, mv, scale, shift, smean, sinv, ACT_LEAKY, out, True,
                           mean_offset=dev(bias), unbiased=True)
        dg0, db0 = f32(rng.standard_normal(C)) * 0 + 0.5, f32(np.full(C, -0.25))
        dgam, dbet = dev(dg0), dev(db0)
        dy = ops.bn_act_any_bwd(dev(y), dev(dout), C, dev(gamma), scale, shift, smean, sinv, ACT_LEAKY, dgam, dbet)
        runs.append((out, mm, mv, dy, dgam, dbet))
    out, mm, mv, dy, dgam, dbet = runs[0]
    # the kernel evaluates fma(scale, y, shift) from float32 scale = gamma / sigma and shift = beta - mean scale, as every
    # BatchNorm kernel of the library does (the LeakyReLU branch is then a function of three stored floats): scale and shift
    # carry half an ulp each, so z carries 2^-24 (|scale y| + |shift|) besides the kernel's own arithmetic -- visible where
    # the two terms cancel (P = 1: var = 0, |scale| = 32 |gamma|, z = beta)
    sc_ref = gamma / np.sqrt(var + R.BN_EPS)
    cancel = 2.0 ** -23 * (np.abs(sc_ref * y) + np.abs(beta - mean * sc_ref)).max()
    close(out, out_ref, "BatchNorm + LeakyReLU", rounding=cancel)
    close(mm, mm_ref, "moving mean")
    close(mv, mv_ref, "moving variance")
    close(dy, dy_ref, "dy", rounding=1e-6 * np.abs(dout).max())     # (P = 1: dy is exactly 0 in exact arithmetic)
    close(dgam, dg0 + dgamma_ref, "dgamma (added)")
    close(dbet, db0 + dbeta_ref, "dbeta (added)")
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    # inference: the moving statistics
    outi = torch.empty((P, C), device="cuda")
    ops.bn_act_any_fwd(dev(y), C, dev(gamma), dev(beta), dev(mm0), dev(mv0), z4(), z4(), z4(), z4(), ACT_LEAKY, outi, False)
    zi = gamma * (y - mm0) / np.sqrt(mv0 + R.BN_EPS) + beta
    close(outi, np.where(zi > 0, zi, 0.1 * zi), "inference", rounding=2e-7 * np.abs(zi).max())
