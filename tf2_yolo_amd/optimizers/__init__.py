"""Optimizers over the flat parameter buffer.

`Adam` mirrors tf.keras.optimizers.Adam (README.md:241: `Adam(lr=1e-4)`): defaults beta_1=0.9,
beta_2=0.999, epsilon=1e-7, bias-corrected, no weight decay; `SGD` mirrors
tf.keras.optimizers.SGD (momentum, Nesterov). Both take the Keras clipping options (`clipnorm`: tf.clip_by_norm per
variable, `global_clipnorm`: tf.clip_by_global_norm, `clipvalue`), the legacy `decay`, and a learning rate that is a number
or a `schedules` object.

Two paths. Without any of the new options an optimizer runs exactly the launches it always ran (one fused kernel per step:
yolo_adam_step / yolo_adam_step_dev, yolo_sgd_step). With AMSGrad, momentum or clipping, the eager step and the recorded
step are ONE sequence -- refresh the device scalars, then norm -> factors -> update (csrc/optim.hip) -- so an eager step and
a replay are the same launches with the same bits. The norm is taken of the gradient the update sees: after the data-parallel
all-reduce, times 1/world."""
import torch

from .. import ops
from . import schedules  # noqa: F401  (tf2_yolo_amd.optimizers.schedules)


def _positive(name, x):
    if x is None:
        return None
    x = float(x)
    if not x > 0.0:
        raise ValueError(f"{name} must be positive, got {x}")
    return x


class Optimizer:
    capturable = False      # has refresh_hyper() / step_captured(): the form a recorded step replays (capture.py)
    _HYPER_SLOTS = 64

    def _init_common(self, learning_rate, lr, clipnorm, clipvalue, global_clipnorm, decay, name):
        self.learning_rate = lr if lr is not None else learning_rate
        given = [(n, v) for n, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm))
                 if v is not None]
        if len(given) > 1:
            raise ValueError(f"at most one of clipnorm, clipvalue and global_clipnorm may be set, got "
                             f"{', '.join(n for n, _ in given)}")
        self.clipnorm, self.clipvalue = _positive("clipnorm", clipnorm), _positive("clipvalue", clipvalue)
        self.global_clipnorm = _positive("global_clipnorm", global_clipnorm)
        self._clip_mode, self._clip_threshold = ops.CLIP_NONE, 0.0
        for mode, t in ((ops.CLIP_NORM, self.clipnorm), (ops.CLIP_GLOBAL, self.global_clipnorm),
                        (ops.CLIP_VALUE, self.clipvalue)):
            if t is not None:
                self._clip_mode, self._clip_threshold = mode, t
        self.decay = float(decay)
        if self.decay < 0.0:
            raise ValueError(f"decay must not be negative, got {self.decay}")
        self.name = name or type(self).__name__
        self.iterations = 0
        self._norm_steps = 0

    # ---- learning rate: a number or a callable schedule(step); assignable between steps ----
    @property
    def learning_rate(self):
        return self._learning_rate

    @learning_rate.setter
    def learning_rate(self, value):
        self._learning_rate = value if callable(value) else float(value)

    lr = learning_rate

    def _lr_now(self):
        """the rate of the step being taken (self.iterations already counts it): schedule(step) and the legacy
        lr / (1 + decay * step), both with step = iterations before the increment, as in Keras"""
        step = self.iterations - 1
        lr = self._learning_rate
        lr = float(lr(step)) if callable(lr) else lr
        if self.decay:
            lr = lr / (1.0 + self.decay * step)
        return lr

    # ---- buffers ----
    def bind(self, net):
        self.net = net
        self._anch = None
        if not self._extended:
            return
        p = net.params
        self._table = ops.ChunkTable([(p.specs[n].offset, p.specs[n].size) for n in p.order])
        if net.has_anchors:     # one Anchor weight per box, as in Keras: every 2 floats are one variable
            self._anch = ops.ChunkTable([(2 * i, 2) for i in range(net.anchors_flat.numel() // 2)])
        self._factors = self._anch_factors = None
        if self._clip_mode in (ops.CLIP_NORM, ops.CLIP_GLOBAL):
            per_var = self._clip_mode == ops.CLIP_NORM
            self._factors = torch.ones(self._table.n_vars if per_var else 1, dtype=torch.float32, device="cuda")
            if self._anch is not None:
                self._anch_factors = (torch.ones(self._anch.n_vars, dtype=torch.float32, device="cuda") if per_var
                                      else self._factors)
        self._norm_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
        self._norm_steps = 0

    def _with_anchors(self):
        return self.net.anchors_trainable and self.net.has_anchors

    def slots(self):
        """name -> tensor of every piece of optimizer state"""
        return {}

    # ---- the device scalars of one step ----
    def _hyper_buffers(self):
        if getattr(self, "_hyper_dev", None) is None:
            # A RING of pinned rows, one per step in flight: the upload is asynchronous and reads its row when the stream
            # gets to it, which can be several steps after the host wrote it (a loop that does not synchronise per step runs
            # ahead of the GPU by as many launches as the queue holds). One row re-written every step -- the form until round
            # 6 -- let step k's upload read the scalars of step k + 1 .. k + 3: a learning rate with the wrong bias
            # correction, a different one from run to run (scripts/step_repro.py with REPRO_SYNC=0: all parameters of
            # YOLOv2-416 differ after the third step by 4e-6 .. 1e-5, the loss after 11 steps takes one of four values).
            self._hyper_host = torch.zeros(self._HYPER_SLOTS, ops.OPT_HYPER, dtype=torch.float32).pin_memory()
            self._hyper_events = [None] * self._HYPER_SLOTS
            self._hyper_dev = torch.zeros(ops.OPT_HYPER, dtype=torch.float32, device="cuda")
        return self._hyper_host, self._hyper_dev

    def _fill_hyper(self, host, grad_scale):
        raise NotImplementedError

    def refresh_hyper(self, grad_scale=1.0):
        """host side of one step whose scalars live on the device: advance the step counter, upload the row of this step
        (ops.OPT_HYPER floats: rate, betas, epsilon, grad_scale, momentum, clip threshold) on the current stream, ahead of
        the launches or of the replay that read it"""
        self.iterations += 1
        ring, dev = self._hyper_buffers()
        slot = self.iterations % self._HYPER_SLOTS
        if self._hyper_events[slot] is not None:
            self._hyper_events[slot].synchronize()   # (its upload of 64 steps ago has long run: returns at once)
        host = ring[slot]
        self._fill_hyper(host, float(grad_scale))
        dev.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._hyper_events[slot] = ev

    # ---- norm -> factors, shared by both optimizers (enqueued eagerly, on a tape or inside a capture alike) ----
    def _enqueue_clip(self, dev):
        """returns (factors of the parameters, factors of the anchors)"""
        if self._clip_mode not in (ops.CLIP_NORM, ops.CLIP_GLOBAL):
            return None, None
        net, anch = self.net, self._anch if self._with_anchors() else None
        ops.grad_sqnorm(net.grads, self._table)
        if anch is not None:
            ops.grad_sqnorm(net.anchor_grads, anch)
        ops.clip_factors(self._table, dev, self._clip_mode, self._factors, norm_out=self._norm_dev, extra=anch)
        if anch is not None and self._clip_mode == ops.CLIP_NORM:
            ops.clip_factors(anch, dev, self._clip_mode, self._anch_factors)
        self._norm_steps += 1
        return self._factors, self._anch_factors

    def _extended_step(self, grad_scale):
        """the eager step of the extended path: the very sequence a recording holds"""
        self.net.before_param_write()
        self.refresh_hyper(grad_scale)
        self.step_captured()
        self.net.mark_params_changed()

    def last_grad_norm(self):
        """global L2 norm of the gradient the last step saw (all-reduced, times 1/world, before clipping), as a Python
        float; None when no norm was computed (no clipnorm / global_clipnorm, or no step yet). Reads the device scalar and
        SYNCHRONISES: for logging, never called by the step."""
        if self._clip_mode not in (ops.CLIP_NORM, ops.CLIP_GLOBAL) or self._norm_steps == 0:
            return None
        return float(self._norm_dev.item())

    def step(self, grad_scale=1.0):
        raise NotImplementedError


class Adam(Optimizer):
    capturable = True

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, decay=0.0, lr=None, name=None):
        self._init_common(learning_rate, lr, clipnorm, clipvalue, global_clipnorm, decay, name)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.amsgrad = bool(amsgrad)
        self.m = self.v = self.vhat = None

    @property
    def _extended(self):
        return self.amsgrad or self._clip_mode != ops.CLIP_NONE

    def bind(self, net):
        super().bind(net)
        self.m = torch.zeros_like(net.params.data)
        self.v = torch.zeros_like(net.params.data)
        self.am = torch.zeros_like(net.anchors_flat)   # trainable anchors (v4): one more small tensor
        self.av = torch.zeros_like(net.anchors_flat)
        self.vhat = torch.zeros_like(net.params.data) if self.amsgrad else None
        self.avhat = torch.zeros_like(net.anchors_flat) if self.amsgrad else None

    def slots(self):
        s = {"m": self.m, "v": self.v, "anchors/m": self.am, "anchors/v": self.av}
        if self.amsgrad:
            s.update({"vhat": self.vhat, "anchors/vhat": self.avhat})
        return s

    def step(self, grad_scale=1.0):
        if self._extended:
            return self._extended_step(grad_scale)
        self.iterations += 1
        lr = self._lr_now()
        self.net.before_param_write()
        ops.adam_step(self.net.params.data, self.net.grads, self.m, self.v, lr, self.iterations,
                      self.beta_1, self.beta_2, self.epsilon, grad_scale=grad_scale, zero_grad=True)
        if self._with_anchors():
            ops.adam_step(self.net.anchors_flat, self.net.anchor_grads, self.am, self.av, lr,
                          self.iterations, self.beta_1, self.beta_2, self.epsilon, grad_scale=grad_scale, zero_grad=True)
        self.net.mark_params_changed()

    # ---- the form a recorded step replays (capture.py): the scalars live in device memory ----
    def _fill_hyper(self, host, grad_scale):
        # (lr_t computed exactly as yolo_adam_step computes it)
        host[0] = ops.adam_lr_t(self._lr_now(), self.iterations, self.beta_1, self.beta_2)
        host[1], host[2], host[3], host[4] = self.beta_1, self.beta_2, self.epsilon, grad_scale
        host[5], host[6] = 0.0, self._clip_threshold

    def step_captured(self):
        """enqueue (eagerly, on a tape or inside a stream capture) the update with the scalars read from the device"""
        _, dev = self._hyper_buffers()
        net = self.net
        if not self._extended:
            ops.adam_step_dev(net.params.data, net.grads, self.m, self.v, dev, zero_grad=True)
            if self._with_anchors():
                ops.adam_step_dev(net.anchors_flat, net.anchor_grads, self.am, self.av, dev, zero_grad=True)
            return
        f, fa = self._enqueue_clip(dev)
        ops.adam_step_clip(net.params.data, net.grads, self.m, self.v, self._table, dev, factors=f,
                           clip_mode=self._clip_mode, vhat=self.vhat, zero_grad=True)
        if self._with_anchors():
            ops.adam_step_clip(net.anchors_flat, net.anchor_grads, self.am, self.av, self._anch, dev, factors=fa,
                               clip_mode=self._clip_mode, vhat=self.avhat, zero_grad=True)


class SGD(Optimizer):
    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, decay=0.0, lr=None, name=None):
        self._init_common(learning_rate, lr, clipnorm, clipvalue, global_clipnorm, decay, name)
        self.momentum = float(momentum)
        if not 0.0 <= self.momentum <= 1.0:
            raise ValueError(f"momentum must be in [0, 1], got {self.momentum}")
        self.nesterov = bool(nesterov)
        self.a = self.aa = None

    @property
    def _extended(self):
        return self.momentum > 0.0 or self._clip_mode != ops.CLIP_NONE

    @property
    def capturable(self):
        return self._extended       # (plain SGD keeps its one eager launch with the rate as an argument)

    def bind(self, net):
        super().bind(net)
        if self.momentum > 0.0:     # (momentum 0 allocates no accumulator)
            self.a = torch.zeros_like(net.params.data)
            self.aa = torch.zeros_like(net.anchors_flat)

    def slots(self):
        return {"momentum": self.a, "anchors/momentum": self.aa} if self.a is not None else {}

    def step(self, grad_scale=1.0):
        if self._extended:
            return self._extended_step(grad_scale)
        self.iterations += 1
        lr = self._lr_now()
        self.net.before_param_write()
        ops.sgd_step(self.net.params.data, self.net.grads, lr, grad_scale=grad_scale, zero_grad=True)
        if self._with_anchors():
            ops.sgd_step(self.net.anchors_flat, self.net.anchor_grads, lr, grad_scale=grad_scale,
                         zero_grad=True)
        self.net.mark_params_changed()

    def _fill_hyper(self, host, grad_scale):
        host[0], host[4], host[5], host[6] = self._lr_now(), grad_scale, self.momentum, self._clip_threshold

    def step_captured(self):
        _, dev = self._hyper_buffers()
        net = self.net
        f, fa = self._enqueue_clip(dev)
        nesterov = self.nesterov and self.a is not None     # (with momentum 0 Nesterov's update IS the plain one)
        ops.sgd_step_clip(net.params.data, net.grads, self._table, dev, accum=self.a, nesterov=nesterov, factors=f,
                          clip_mode=self._clip_mode, zero_grad=True)
        if self._with_anchors():
            ops.sgd_step_clip(net.anchors_flat, net.anchor_grads, self._anch, dev, accum=self.aa, nesterov=nesterov,
                              factors=fa, clip_mode=self._clip_mode, zero_grad=True)
