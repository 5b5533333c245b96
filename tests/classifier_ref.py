"""float64 NumPy statement of the classifier top: GlobalAveragePooling2D, Dense + softmax, Keras' categorical cross-entropy on
probabilities and categorical accuracy, each with its backward. tests/test_classifier_cpu.py checks it against torch float64
autograd on CASES; the GPU tests compare the kernels of csrc/classify.hip against this file.

Layouts are the library's: x [N,H,W,C], g [N,C], W [K,C], b [K], p / t [N,K]."""
import numpy as np

EPS = 1e-7     # Keras backend epsilon: categorical_crossentropy clips q to [EPS, 1 - EPS]

GAP_CASES = [(1, 1, 1, 64), (2, 2, 2, 1024), (3, 3, 5, 10), (5, 7, 7, 3), (2, 13, 13, 1000)]     # (N, H, W, C)
DENSE_CASES = [(1, 64, 1), (2, 1024, 1000), (5, 1024, 3), (3, 96, 65)]                            # (N, C, K)
SOFTMAX_CASES = [(4, 10, 10), (2, 3, 3)]                                                         # the null-weights form
CASES = {"gap": GAP_CASES, "dense": DENSE_CASES, "softmax": SOFTMAX_CASES}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def gap_fwd(x):
    return f64(x).mean(axis=(1, 2))


def gap_bwd(dg, H, W):
    dg = f64(dg)
    return np.broadcast_to(dg[:, None, None, :] / (H * W), (dg.shape[0], H, W, dg.shape[1])).copy()


def softmax(z):
    z = f64(z)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def dense_softmax_fwd(g, W=None, b=None):
    """(logits, p); W = b = None: the softmax of g itself"""
    z = f64(g) if W is None else f64(g) @ f64(W).T + f64(b)
    return z, softmax(z)


def dense_softmax_bwd(dp, p, g, W=None):
    """(dz, dg, dW, db); without weights dg = dz and dW = db = None"""
    dp, p = f64(dp), f64(p)
    dz = p * (dp - (p * dp).sum(axis=1, keepdims=True))
    if W is None:
        return dz, dz, None, None
    return dz, dz @ f64(W), dz.T @ f64(g), dz.sum(axis=0)


def cce(t, p):
    """Keras categorical_crossentropy(t, p) on probabilities, averaged over the batch"""
    t, p = f64(t), f64(p)
    q = p / p.sum(axis=1, keepdims=True)
    return float((-(t * np.log(np.clip(q, EPS, 1 - EPS))).sum(axis=1)).mean())


def cce_grad(t, p, grad_scale=1.0):
    """d cce / d p, times grad_scale; the clip passes no gradient outside [EPS, 1 - EPS]"""
    t, p = f64(t), f64(p)
    S = p.sum(axis=1, keepdims=True)
    q = p / S
    inside = (q >= EPS) & (q <= 1 - EPS)
    dq = np.where(inside, -t / np.clip(q, EPS, 1 - EPS), 0.0)          # d(-sum t log clip(q)) / dq
    return grad_scale * (dq - (dq * q).sum(axis=1, keepdims=True)) / S / t.shape[0]


def accuracy(t, p):
    """categorical accuracy; np.argmax, like tf.argmax, takes the first maximum"""
    return float((np.argmax(f64(t), axis=1) == np.argmax(f64(p), axis=1)).mean())


def top_gap(rows):
    """smallest difference between the two largest entries of every row"""
    s = np.sort(f64(rows), axis=1)
    return s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.full(s.shape[0], np.inf)


def one_hot(labels, K):
    t = np.zeros((len(labels), K))
    t[np.arange(len(labels)), labels] = 1.0
    return t


def top_from_features(F, W, b, t):
    """the whole top of a Dense classifier from the trunk's feature map F [N,H,W,C]: W is the Keras kernel [C,K].
    Returns dict(p, loss, dW [C,K], db, dF)."""
    g = gap_fwd(F)
    _, p = dense_softmax_fwd(g, f64(W).T, b)
    dp = cce_grad(t, p)
    _, dg, dW, db = dense_softmax_bwd(dp, p, g, f64(W).T)
    return {"p": p, "loss": cce(t, p), "dW": dW.T, "db": db, "dF": gap_bwd(dg, F.shape[1], F.shape[2])}


# ---- BatchNormalization + LeakyReLU(0.1) over any channel count (darknet19's class convolution) ---------------------------
BN_EPS, BN_MOMENTUM = 1e-3, 0.99     # Keras BatchNormalization defaults
BN_CASES = [(1, 3), (16, 3), (16, 2), (300, 10), (1000, 5), (37, 1)]      # (P, C): one pixel, fewer / more than a workgroup


def bn_leaky_fwd(y, gamma, beta):
    """training-mode forward on y [P,C]: (out, mean, biased variance, xhat)"""
    y = f64(y)
    mean, var = y.mean(axis=0), y.var(axis=0)
    xhat = (y - mean) / np.sqrt(var + BN_EPS)
    z = f64(gamma) * xhat + f64(beta)
    return np.where(z > 0, z, 0.1 * z), mean, var, xhat


def bn_leaky_bwd(y, dout, gamma, beta):
    """(dy, dgamma, dbeta) of bn_leaky_fwd"""
    _, _, var, xhat = bn_leaky_fwd(y, gamma, beta)
    z = f64(gamma) * xhat + f64(beta)
    dz = np.where(z > 0, 1.0, 0.1) * f64(dout)
    dy = f64(gamma) / np.sqrt(var + BN_EPS) * (dz - dz.mean(axis=0) - xhat * (dz * xhat).mean(axis=0))
    return dy, (dz * xhat).sum(axis=0), dz.sum(axis=0)


def bn_moving(moving_mean, moving_var, mean, var, P, unbiased, offset=0.0):
    fed = var * P / (P - 1) if (unbiased and P > 1) else var
    return (f64(moving_mean) * BN_MOMENTUM + (mean + offset) * (1 - BN_MOMENTUM),
            f64(moving_var) * BN_MOMENTUM + fed * (1 - BN_MOMENTUM))
