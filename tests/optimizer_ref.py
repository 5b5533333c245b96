"""Reference optimizers for the tests: the Keras (optimizer_v2) update rules RESTATED in float64 NumPy.

TensorFlow is not available where these tests run, so nothing here calls Keras: every formula below is written from the
documented Keras semantics --

  clipnorm          tf.clip_by_norm per variable:      g_v * clipnorm / max(||g_v||, clipnorm)
  global_clipnorm   tf.clip_by_global_norm:            g * clip / max(||g||, clip), ||g|| over all variables
  clipvalue         tf.clip_by_value:                  clamp(g, -clipvalue, +clipvalue)
  Adam              m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; lr_t = lr sqrt(1-b2^t) / (1-b1^t);
                    p -= lr_t m / (sqrt(v) + eps);     amsgrad: vhat = max(vhat, v), p -= lr_t m / (sqrt(vhat) + eps)
  SGD               ResourceApplyKerasMomentum:        a = mu a - lr g; p += a, or with nesterov p += mu a - lr g;
                    mu = 0: p -= lr g

-- all on g = (all-reduced gradient) * grad_scale. Variables are (offset, size) slices of flat buffers; elements outside every
variable (the padding) are never read into a norm and never written."""
import numpy as np

# the variable sizes the kernel tests and the table test use: one element, a scalar tail, exactly / just over one 64-float
# alignment unit, more than one float4 pass with a tail, and several chunks with a partial last one
SIZES = (1, 3, 64, 65, 4099, 70000)


def layout(sizes=SIZES, align=64):
    """(offset, size) pairs at `align`-float aligned offsets, as ParamStore lays variables out, and the padded total"""
    out, total = [], 0
    for s in sizes:
        out.append((total, s))
        total += (s + align - 1) // align * align
    return out, total


def mask(variables, total):
    m = np.zeros(total, dtype=bool)
    for off, size in variables:
        m[off:off + size] = True
    return m


def sq_norms(g, variables):
    """per-variable and global squared L2 norms of float32 data, in float64"""
    g = np.asarray(g, dtype=np.float64)
    per = np.array([np.sum(g[o:o + s] ** 2) for o, s in variables])
    return per, float(np.sum(per))


def clipped(g, variables, grad_scale=1.0, clipnorm=None, global_clipnorm=None, clipvalue=None):
    """the gradient the update sees (float64, zero in the padding) and the global norm of grad_scale * g"""
    g = np.asarray(g, dtype=np.float64) * grad_scale
    out = np.zeros_like(g)
    per, tot = sq_norms(g, variables)
    gnorm = np.sqrt(tot)
    for k, (o, s) in enumerate(variables):
        x = g[o:o + s]
        if clipnorm is not None:
            x = x * (clipnorm / max(np.sqrt(per[k]), clipnorm))
        elif global_clipnorm is not None:
            x = x * (global_clipnorm / max(gnorm, global_clipnorm))
        elif clipvalue is not None:
            x = np.clip(x, -clipvalue, clipvalue)
        out[o:o + s] = x
    return out, gnorm


class AdamRef:
    def __init__(self, p, variables, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, amsgrad=False, **clip):
        self.p = np.asarray(p, dtype=np.float64).copy()
        self.vars, self.mask = variables, mask(variables, len(self.p))
        self.m, self.v, self.vhat = np.zeros_like(self.p), np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps, self.amsgrad, self.clip, self.t = lr, b1, b2, eps, amsgrad, clip, 0

    def step(self, g, grad_scale=1.0):
        self.t += 1
        gg, gnorm = clipped(g, self.vars, grad_scale, **self.clip)
        k = self.mask
        self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * gg[k]
        self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * gg[k] ** 2
        lr_t = self.lr * np.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        if self.amsgrad:
            self.vhat[k] = np.maximum(self.vhat[k], self.v[k])
            self.p[k] -= lr_t * self.m[k] / (np.sqrt(self.vhat[k]) + self.eps)
        else:
            self.p[k] -= lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
        return gnorm


class SGDRef:
    def __init__(self, p, variables, lr=1e-2, momentum=0.0, nesterov=False, **clip):
        self.p = np.asarray(p, dtype=np.float64).copy()
        self.vars, self.mask = variables, mask(variables, len(self.p))
        self.a = np.zeros_like(self.p)
        self.lr, self.mu, self.nesterov, self.clip = lr, momentum, nesterov, clip

    def step(self, g, grad_scale=1.0):
        gg, gnorm = clipped(g, self.vars, grad_scale, **self.clip)
        k = self.mask
        if self.mu == 0.0:
            self.p[k] -= self.lr * gg[k]
            return gnorm
        self.a[k] = self.mu * self.a[k] - self.lr * gg[k]
        if self.nesterov:
            self.p[k] += self.mu * self.a[k] - self.lr * gg[k]
        else:
            self.p[k] += self.a[k]
        return gnorm


# ---- schedules (closed forms of tf.keras.optimizers.schedules) and the legacy decay ----
def exponential_decay(step, lr0, decay_steps, rate, staircase=False):
    p = step / decay_steps
    return lr0 * rate ** (np.floor(p) if staircase else p)


def piecewise_constant(step, boundaries, values):
    return values[int(np.searchsorted(np.asarray(boundaries), step, side="left"))]


def cosine_decay(step, lr0, decay_steps, alpha=0.0):
    s = min(step, decay_steps)
    return lr0 * ((1 - alpha) * 0.5 * (1 + np.cos(np.pi * s / decay_steps)) + alpha)


def legacy_decay(step, lr0, decay):
    return lr0 / (1.0 + decay * step)
