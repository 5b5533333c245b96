"""Static-graph executor for the YOLO training / inference hot path.

The reference builds tf.keras graphs (yolov3/models/*.py etc.) and lets Keras run
forward / autodiff / optimizer. Here a model is a flat list of units built once by
`GraphBuilder`; `Network.forward` / `Network.backward` walk it and enqueue the HIP kernels of
libyolo_hip.so on the current stream. Design points (MI355X-first):

  * NHWC fp32 activations, KRSC filters; all trainable parameters live in ONE flat buffer
    (`params`), with matching flat `grads`, Adam `m`/`v`: one optimizer launch per step and
    contiguous gradient buckets for the RCCL all-reduce (reverse construction order ==
    backward completion order).
  * every conv output and activation of a training step stays resident (288 GB HBM: no
    recompute, no offload); buffers are allocated once per batch size and reused.
  * conv+BN+activation(+residual Add) is one unit: conv kernel (BN statistics accumulated in
    fp64), a per-channel finalize, one fused normalise+activate(+add) pass.
  * gradient fan-out (residual skips, FPN taps) is resolved with "first writer aliases,
    later writers accumulate in place", so identity branches cost no copies.
"""
import math

import contextlib

import numpy as np
import torch

from . import ops
from . import plan
from . import tape
from ._lib import ACT_LEAKY, ACT_LINEAR, ACT_MISH, YoloHipError
from .plan import AUX_WORDS, has_filter

ACT_NAMES = {ACT_LINEAR: "linear", ACT_LEAKY: "leaky", ACT_MISH: "mish"}


# --------------------------------------------------------------------------------------------
# parameter store
# --------------------------------------------------------------------------------------------
class ParamSpec:
    __slots__ = ("name", "shape", "offset", "size", "init", "trainable")

    def __init__(self, name, shape, offset, init, trainable):
        self.name, self.shape, self.offset = name, tuple(shape), offset
        self.size = int(np.prod(shape))
        self.init, self.trainable = init, trainable


class ParamStore:
    """Flat fp32 storage. Offsets are padded to 64 floats so every slice is 256-B aligned."""

    def __init__(self):
        self.specs = {}
        self.order = []
        self.total = 0

    def add(self, name, shape, init):
        if name in self.specs:
            raise ValueError(f"duplicate parameter {name}")
        spec = ParamSpec(name, shape, self.total, init, True)
        self.specs[name] = spec
        self.order.append(name)
        self.total += (spec.size + 63) // 64 * 64
        return spec

    def materialize(self, device, rng):
        host = np.zeros(self.total, dtype=np.float32)
        for name in self.order:
            s = self.specs[name]
            host[s.offset:s.offset + s.size] = s.init(rng, s.shape).reshape(-1)
        self.data = torch.from_numpy(host).to(device)
        return self.data

    def view(self, name):
        s = self.specs[name]
        return self.data[s.offset:s.offset + s.size]


def init_zeros(rng, shape):
    return np.zeros(shape, dtype=np.float32)


def init_ones(rng, shape):
    return np.ones(shape, dtype=np.float32)


def he_normal_krsc(rng, shape):
    """Keras he_normal: truncated normal (|z| <= 2), stddev = sqrt(2/fan_in)/0.87962566
    (SURVEY.md Appendix B); shape is KRSC so fan_in = kh*kw*Cin."""
    cout, kh, kw, cin = shape
    std = math.sqrt(2.0 / (kh * kw * cin)) / 0.87962566103423978
    z = rng.standard_normal(shape)
    bad = np.abs(z) > 2.0
    while bad.any():
        z[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(z) > 2.0
    return (z * std).astype(np.float32)


def random_normal_002(rng, shape):
    """yolov4/models/backbone.py:68: RandomNormal(mean=0.0, stddev=0.02)."""
    return (rng.standard_normal(shape) * 0.02).astype(np.float32)


# --------------------------------------------------------------------------------------------
# graph description
# --------------------------------------------------------------------------------------------
class TensorRef:
    """Symbolic activation: spatial shape without the batch dimension."""
    __slots__ = ("tid", "h", "w", "c", "name", "producer", "rank2")

    def __init__(self, tid, h, w, c, name, producer=None, rank2=False):
        self.tid, self.h, self.w, self.c, self.name, self.producer = tid, h, w, c, name, producer
        self.rank2 = rank2     # [N, C]: behind GlobalAveragePooling2D (h = w = 1)

    @property
    def shape(self):
        return (None, self.c) if self.rank2 else (None, self.h, self.w, self.c)


class Unit:
    kind = "unit"
    residual = None

    def __init__(self, name):
        self.name = name
        self.inputs = []
        self.out = None

    def param_names(self):
        return []


class ConvUnit(Unit):
    """conv [+bias] [+BatchNorm] [+activation] [+residual add]."""
    kind = "conv"

    def __init__(self, name, src, cout, k, stride, padding, bn, act, bias, residual, kernel_init):
        super().__init__(name)
        self.src, self.cout, self.k, self.stride, self.padding = src, cout, k, stride, padding
        self.bn, self.act, self.bias, self.residual = bn, act, bias, residual
        self.kernel_init = kernel_init
        self.inputs = [src] + ([residual] if residual is not None else [])


class HeadUnit(Unit):
    """All per-anchor 1x1 head convs of one output level fused into one [A*(5+C)] x Cin GEMM
    plus the per-channel activations (yolov3/models/__init__.py:40-65)."""
    kind = "head"
    k = stride = 1      # the questions a ConvUnit answers, for code that treats both alike
    padding = "same"
    bn = False
    bias = True

    def __init__(self, name, src, A, C, version, anchors, level, kernel_init):
        super().__init__(name)
        self.src, self.A, self.C, self.version, self.level = src, A, C, version, level
        self.cout = (5 * A + C) if version == 1 else A * (5 + C)
        self.kernel_init = kernel_init
        self.anchors = [tuple(map(float, a)) for a in anchors] if anchors is not None else None
        self.inputs = [src]


class UpsampleUnit(Unit):
    kind = "upsample"

    def __init__(self, name, src):
        super().__init__(name)
        self.src = src
        self.inputs = [src]


class ConcatUnit(Unit):
    kind = "concat"

    def __init__(self, name, srcs):
        super().__init__(name)
        self.srcs = list(srcs)
        self.inputs = list(srcs)


class MaxPoolUnit(Unit):
    kind = "maxpool"

    def __init__(self, name, src, k, stride, padding):
        super().__init__(name)
        self.src, self.k, self.stride, self.padding = src, k, stride, padding
        self.inputs = [src]


class SpaceToDepthUnit(Unit):
    kind = "space_to_depth"

    def __init__(self, name, src):
        super().__init__(name)
        self.src = src
        self.inputs = [src]


class GapUnit(Unit):
    """GlobalAveragePooling2D: [N,H,W,C] -> [N,C]"""
    kind = "gap"

    def __init__(self, name, src):
        super().__init__(name)
        self.src = src
        self.inputs = [src]


class DenseSoftmaxUnit(Unit):
    """Dense(K, activation="softmax") on a [N,C] tensor. The kernel is stored [K][C] (the rows the kernels stream); the
    Keras-facing layout is [C,K]."""
    kind = "dense_softmax"

    def __init__(self, name, src, K):
        super().__init__(name)
        self.src, self.K = src, K
        self.inputs = [src]


class SoftmaxUnit(Unit):
    """Softmax() on a [N,C] tensor (darknet19's last layer)"""
    kind = "softmax"

    def __init__(self, name, src):
        super().__init__(name)
        self.src = src
        self.inputs = [src]


def he_normal_dense(rng, shape):
    """Keras he_normal of a Dense kernel stored [K][C]: fan_in = C"""
    k, c = shape
    return he_normal_krsc(rng, (k, 1, 1, c)).reshape(k, c)


class GraphBuilder:
    """Functional-style builder, one call per reference layer group."""

    def __init__(self, input_shape, kernel_init=he_normal_krsc):
        h, w, c = input_shape
        self.tensors = []
        self.units = []
        self.kernel_init = kernel_init
        self.input = self._tensor(h, w, c, "input")
        self.outputs = []

    def _tensor(self, h, w, c, name, producer=None):
        t = TensorRef(len(self.tensors), h, w, c, name, producer)
        self.tensors.append(t)
        return t

    def _push(self, unit, h, w, c):
        unit.out = self._tensor(h, w, c, unit.name, unit)
        self.units.append(unit)
        return unit.out

    def conv(self, src, cout, k, name, stride=1, padding=None, bn=True, act=ACT_LEAKY, bias=False, residual=None,
             kernel_init=None):
        if padding is None:
            padding = "same"
        d = ops.conv_desc((1, src.h, src.w, src.c), cout, k, k, stride, padding)
        if residual is not None and (residual.h, residual.w, residual.c) != (d.Ho, d.Wo, cout):
            raise ValueError(f"{name}: residual shape mismatch")
        u = ConvUnit(name, src, cout, k, stride, padding, bn, act, bias, residual, kernel_init or self.kernel_init)
        return self._push(u, d.Ho, d.Wo, cout)

    def upsample(self, src, name):
        return self._push(UpsampleUnit(name, src), src.h * 2, src.w * 2, src.c)

    def concat(self, srcs, name):
        h, w = srcs[0].h, srcs[0].w
        for s in srcs:
            if (s.h, s.w) != (h, w):
                raise ValueError(f"{name}: concat of different spatial sizes")
        return self._push(ConcatUnit(name, srcs), h, w, sum(s.c for s in srcs))

    def maxpool(self, src, k, name, stride=None, padding="valid"):
        stride = stride or k
        if padding == "same":
            ho, wo = -(-src.h // stride), -(-src.w // stride)
        else:
            ho, wo = (src.h - k) // stride + 1, (src.w - k) // stride + 1
        return self._push(MaxPoolUnit(name, src, k, stride, padding), ho, wo, src.c)

    def space_to_depth(self, src, name):
        return self._push(SpaceToDepthUnit(name, src), src.h // 2, src.w // 2, src.c * 4)

    def head(self, src, A, C, version, anchors, name, level):
        u = HeadUnit(name, src, A, C, version, anchors, level, self.kernel_init)
        out = self._push(u, src.h, src.w, u.cout)
        self.outputs.append(out)
        return out

    def gap(self, src, name):
        out = self._push(GapUnit(name, src), 1, 1, src.c)
        out.rank2 = True
        return out

    def dense_softmax(self, src, K, name):
        if not src.rank2:
            raise ValueError(f"{name}: Dense takes a [N, C] tensor (put gap() in front)")
        out = self._push(DenseSoftmaxUnit(name, src, int(K)), 1, 1, int(K))
        out.rank2 = True
        return out

    def softmax(self, src, name):
        if not src.rank2:
            raise ValueError(f"{name}: Softmax takes a [N, C] tensor (put gap() in front)")
        out = self._push(SoftmaxUnit(name, src), 1, 1, src.c)
        out.rank2 = True
        return out

    def output(self, t):
        """mark any tensor as a network output (heads register themselves)"""
        if t not in self.outputs:
            self.outputs.append(t)
        return t


def count_params(builder):
    """(trainable, non_trainable) parameter counts of a built graph (no device needed)."""
    train = state = 0
    for u in builder.units:
        if has_filter(u):
            train += u.cout * u.k * u.k * u.src.c + (u.cout if u.bias else 0) + (2 * u.cout if u.bn else 0)
            state += 2 * u.cout if u.bn else 0
        elif u.kind == "dense_softmax":
            train += u.K * u.src.c + u.K
    return train, state


def conv_flops_per_image(builder):
    """2*Ho*Wo*Cout*Cin*kh*kw summed over every conv (head convs included): SURVEY.md section 8d."""
    total = 0
    for u in builder.units:
        if has_filter(u):
            total += 2 * u.out.h * u.out.w * u.cout * u.src.c * u.k * u.k
    return total


# --------------------------------------------------------------------------------------------
# runtime
# --------------------------------------------------------------------------------------------
_EPILOGUES = {ACT_LEAKY: ops.EPI_AFFINE_LEAKY, ACT_MISH: ops.EPI_AFFINE_MISH}


def _epilogue(u):
    """the fused-epilogue code of a conv + BN unit's inference form: folded BatchNormalization + its activation"""
    return _EPILOGUES.get(u.act, ops.EPI_AFFINE)


class Network:
    def __init__(self, builder, device="cuda", seed=1234, unbiased_moving_var=True):
        if not torch.cuda.is_available():
            raise YoloHipError("tf2_yolo_amd needs a HIP device: there is no CPU fallback")
        self.device = torch.device(device)
        if self.device.index is not None and self.device.index != torch.cuda.current_device():
            raise YoloHipError(f"Network(device={device!r}): the kernels launch on the current device "
                               f"(cuda:{torch.cuda.current_device()}); call torch.cuda.set_device first "
                               "(one process per GPU)")
        self.tensors = builder.tensors
        self.units = builder.units
        self.input = builder.input
        self.outputs = list(builder.outputs)
        self.unbiased_moving_var = unbiased_moving_var
        # the switches (plan.Options says what each one does) as _overlap_wgrad, _prep_beside, _stem_fused, _bn_tight,
        # _res_from_planes, _use_infer_graph, _fuse_infer, _concat_grad_slices, _dyp_per_layer, _bn_fold, _bn_fused_reduce,
        # _pool_fuse, _concat_planes, _infer_onepass, _infer_small_fuse; _overlap_wgrad is read at every call (bench.py sets it)
        self._opts = plan.Options.from_env()
        for k, v in vars(self._opts).items():
            setattr(self, "_" + k, v)
        g = self._plan = plan.plan_graph(self.units, self.tensors, self.input, self.outputs, self._opts)
        self._needs_grad, self._n_consumers = g.needs_grad, g.n_consumers
        self._bound_alias, self._up_producer = g.bound_alias, g.up_producer
        self.params = ParamStore()   # trainable
        self.state = ParamStore()    # BN moving statistics (not trainable, not all-reduced)
        self._declare_params()
        rng = np.random.default_rng(seed)
        self.params.materialize(self.device, rng)
        self.state.materialize(self.device, rng)
        self.grads = torch.zeros_like(self.params.data)
        self._init_anchors()
        ops.create_side_streams(self.device)   # this device's filter-gradient / communication streams (fixed creation order)
        ops.ensure_conv_workspace()   # scratch of the persistent (stream-K) window kernel: small-batch launches
        ops.ensure_wgrad_workspace()  # slabs of the atomics-free filter / bias gradient reductions
        self._alloc_planned_buffers(g)
        self._wT_valid = self._wp_valid = self._wTp_valid = False
        self._jobs_wp = self._jobs_wTp = self._jobs_wT = None
        self._wp_event = self._wT_event = None
        self._infer_graphs = {}
        self._wgrad_stream = None
        self._wgrad_pending = False
        self.batch = None
        self.act = {}
        self.training = False
        self._precision = "fp32"   # of the forward in progress: "fp16" = one MFMA pass, inference only (forward())
        self.grad_ready_hook = None   # called as hook(unit) after a unit's parameter grads are enqueued
        self.backward_begin_hook = None   # called at the start of backward (the gradient reducer's time origin)
        self._infer_scale_valid = False
        # A one-pass inference unit leaves the bound of its result as one word per workgroup of its last launch (their
        # maximum; include/yolo_hip.h: yolo_conv2d_fwd_infer_unit): _tword_n[tid] words of the tensor's row, allocated on first use
        self._twords = None
        self._tword_n = {}
        self._xplanes_infer = {}
        for u in self.units:
            u.concat_reads_through = False

    # ---- construction -------------------------------------------------------------------
    def _declare_params(self):
        for u in self.units:
            if u.kind == "conv":
                u.p_kernel = self.params.add(f"{u.name}_conv/kernel", (u.cout, u.k, u.k, u.src.c), u.kernel_init)
                u.p_bias = self.params.add(f"{u.name}_conv/bias", (u.cout,), init_zeros) if u.bias else None
                if u.bn:
                    u.p_gamma = self.params.add(f"{u.name}_bn/gamma", (u.cout,), init_ones)
                    u.p_beta = self.params.add(f"{u.name}_bn/beta", (u.cout,), init_zeros)
                    u.s_mean = self.state.add(f"{u.name}_bn/moving_mean", (u.cout,), init_zeros)
                    u.s_var = self.state.add(f"{u.name}_bn/moving_variance", (u.cout,), init_ones)
            elif u.kind == "head":
                u.p_kernel = self.params.add(f"{u.name}/kernel", (u.cout, 1, 1, u.src.c), u.kernel_init)
                u.p_bias = self.params.add(f"{u.name}/bias", (u.cout,), init_zeros)
            elif u.kind == "dense_softmax":
                u.p_kernel = self.params.add(f"{u.name}/kernel", (u.K, u.src.c), he_normal_dense)
                u.p_bias = self.params.add(f"{u.name}/bias", (u.K,), init_zeros)

    def _init_anchors(self):
        """head anchors (v2-v4): views into ONE flat buffer with a gradient twin, so that trainable anchors
        (yolov4/__init__.py:147-159) are one more small optimizer tensor"""
        self._anchors_dev, self._anchor_grad_views = {}, {}
        heads = [u for u in self.units if u.kind == "head" and u.anchors is not None]
        n_anch = sum(2 * len(u.anchors) for u in heads)
        self.anchors_flat = torch.zeros(max(n_anch, 1), device=self.device, dtype=torch.float32)
        self.anchor_grads = torch.zeros_like(self.anchors_flat)
        self.anchors_trainable = False
        off = 0
        for u in heads:
            n = 2 * len(u.anchors)
            self.anchors_flat[off:off + n] = torch.tensor(np.array(u.anchors, dtype=np.float32).reshape(-1))
            self._anchors_dev[u.name] = self.anchors_flat[off:off + n]
            self._anchor_grad_views[u.name] = self.anchor_grads[off:off + n]
            off += n
        self.has_anchors = n_anch > 0

    def _alloc_planned_buffers(self, g):
        """the flat buffers whose layout plan.plan_graph made, and each unit's constant views into them"""
        dev = self.device
        self._wT = torch.empty(g.wT_total, device=dev, dtype=torch.float32)
        self._bn_f32 = torch.zeros(max(g.bn_f32_total, 1), device=dev, dtype=torch.float32)
        self._bn_f64 = torch.zeros(max(g.bn_f64_total, 1), device=dev, dtype=torch.float64)
        self._bn_stats_total = g.bn_stats_total
        self._wplanes = torch.empty(g.wplanes_total, device=dev, dtype=torch.uint8) if g.wplanes_total else None
        self._aux = torch.zeros(g.aux_total, device=dev, dtype=torch.int32)
        self._tbound = self._aux[g.tbound_off:].view(torch.float32)
        self._tb = [self._tbound[i:i + 1] for i in range(len(self.tensors))]   # a tensor's bound float
        self._pred = torch.zeros(g.pred_total, device=dev, dtype=torch.float32)
        for u in self.units:
            a = u.aux_off
            u.bound = self._aux[a:a + 1]             # bound of the BatchNorm output
            u.red_bound = self._aux[a + 1:a + 69]    # the 68 words of yolo_bn_act_bwd_reduce_bound
            u.tickets = self._aux[a + 69:a + 69 + ops.BN_FOLD_TICKET_WORDS]
            u.pred = self._pred[u.pred_off:u.pred_off + 2]
            if u.kind == "conv" and u.bn:
                u.amax = self._aux[a + AUX_WORDS:a + AUX_WORDS + u.cout]   # per-channel max|conv out|
            if not has_filter(u):
                continue
            u.wT = self._wT[u.wT_off:u.wT_off + u.cout * u.k * u.k * u.src.c]
            u.wp = self._wplanes[u.wp_off:u.wp_off + u.wp_bytes] if u.planes_fwd else None
            u.wTp = self._wplanes[u.wTp_off:u.wTp_off + u.wTp_bytes] if u.planes_dgrad else None
            if u.cpad:
                u.wTp_pad = self._wplanes[u.wTp_pad_off:u.wTp_pad_off + u.wTp_pad_bytes]
                n = u.cpad * u.src.c
                u.w_pad = torch.zeros(n, device=dev, dtype=torch.float32)    # [cpad][cin], zero rows past out.c
                u.wT_pad = torch.empty(n, device=dev, dtype=torch.float32)   # [cin][cpad]
                u.dw_pad = torch.empty(n, device=dev, dtype=torch.float32)   # filter-gradient scratch

    @property
    def num_params(self):
        return sum(self.params.specs[n].size for n in self.params.order)

    @property
    def num_state(self):
        return sum(self.state.specs[n].size for n in self.state.order)

    # ---- buffers ------------------------------------------------------------------------
    def allocate(self, N):
        if self.batch == N:
            return
        # every conv kernel addresses its operands through buffer descriptors with 32-bit offsets (the planes kernels check
        # it per launch, the register-staged ones do not): say so HERE, with the largest batch that fits, instead of
        # failing -- or wrapping around -- inside forward. 4 GiB per ACTIVATION is 192 images of YOLOv3-416 per GPU; a
        # larger global batch is what data parallelism is for.
        worst = max((t.h * t.w * t.c * 4 for t in self.tensors), default=0)
        if worst and N * worst + (1 << 20) >= (1 << 32):
            raise YoloHipError(f"batch {N}: the largest activation ({worst / 2 ** 20:.1f} MiB per image) would exceed the "
                               f"4 GiB a conv operand may span; the largest per-GPU batch for this model is "
                               f"{((1 << 32) - (1 << 20)) // worst - 1}")
        self.batch = N
        self.alloc_gen = getattr(self, "alloc_gen", 0) + 1   # captured step graphs (capture.py) belong to one allocation
        self._infer_graphs = {}   # captured graphs point into the buffers re-allocated below
        self.act = {}
        bp = plan.plan_batch(self.units, N, self._opts)

        def new(u, dtype=torch.float32):
            return torch.empty((N, u.out.h, u.out.w, u.out.c), device=self.device, dtype=dtype)

        def new_bytes(n, make=torch.empty):
            return make(n, device=self.device, dtype=torch.uint8)
        for u in self.units:
            u.bnred = None
            if u.kind == "conv":
                u.desc = bp.desc[u.name]
                u.y = new(u)
                u.a = new(u) if (u.bn or u.act != ACT_LINEAR) else u.y
                self.act[u.out.tid] = u.a
            elif u.kind == "head":
                u.desc, u.desc_pad = bp.desc[u.name], bp.desc_pad.get(u.name)
                u.t = new(u)
                u.yact = new(u)
                self.act[u.out.tid] = u.yact
            elif u.kind in ("gap", "dense_softmax", "softmax"):
                # [N, C] tensors; dsrc = the gradient this unit writes for its input (None: the input needs none)
                u.buf = torch.empty((N, u.out.c), device=self.device, dtype=torch.float32)
                src_shape = (N, u.src.h, u.src.w, u.src.c) if u.kind == "gap" else (N, u.src.c)
                u.dsrc = (torch.empty(src_shape, device=self.device, dtype=torch.float32)
                          if self._needs_grad[u.src.tid] else None)
                if u.kind == "dense_softmax":
                    u.logits, u.dz = torch.empty_like(u.buf), torch.empty_like(u.buf)   # pre-softmax values, their gradient
                self.act[u.out.tid] = u.buf
            else:
                u.buf = new(u)
                if u.kind == "maxpool":
                    u.argmax = new(u, torch.int32)
                    u.pad_t, u.pad_l = bp.pool_pad[u.name]
                self.act[u.out.tid] = u.buf
        # the BatchNormalization-backward reductions made by data gradients (plan: _plan_fused_reduce, plan_batch)
        by_name = {u.name: u for u in self.units}
        for name, cap in bp.bnred_cap.items():
            p = by_name[name]
            scale, shift, smean, sinv, _, _ = self._bn_bufs(p)
            p.bnred = ops.BnReduce(p.y, scale, shift, smean, sinv, p.act,
                                   torch.empty(cap * 2 * p.cout, device=self.device, dtype=torch.float32), cap, p.red_bound)
            p.bnred_done = False
        # planes of the activations that feed planes-capable convs (kept from forward for the filter gradient)
        self._xplanes = {tid: new_bytes(n, torch.zeros) for tid, n in bp.xplanes_bytes.items()}
        self._xplanes_infer = {}
        self._xp_valid = set()
        # planes of the current layer's dy in backward: every planes layer owns its buffer (Options.dyp_per_layer), or
        # two scratch buffers are used alternately: the filter gradient of layer L may still be reading its dy planes on the
        # second stream while layer L-1 produces its own (with own buffers _next_dyp_buffer creates the pair on demand)
        dyp = self._dyp_shared_bytes = bp.dyp_shared_bytes
        self._dyplanes2 = [None, None] if self._dyp_per_layer else [new_bytes(dyp) if dyp else None for _ in range(2)]
        self._dyp_events = [None, None]
        self._dyp_idx = 0
        self._dyp_own = {name: new_bytes(n) for name, n in bp.dyp_own_bytes.items()}

    def _tb_row(self, tid):
        if self._twords is None:
            self._twords = torch.zeros((max(len(self.tensors), 1) + 1) * ops.INFER_BOUND_WORDS, device=self.device,
                                       dtype=torch.int32)
        return self._twords[tid * ops.INFER_BOUND_WORDS:(tid + 1) * ops.INFER_BOUND_WORDS]

    def _tb_float(self, tid):
        """the recorded bound of tensor tid as ONE device float (folds the words of a one-pass inference unit once)"""
        n = self._tword_n.pop(tid, 0)
        if n:
            ops.fold_bound(self._tb_row(tid)[:n], self._tb[tid])
        return self._tb[tid]

    def _tb_words(self, tid):
        """the recorded bound of tensor tid as the one-pass units take it: the words such a unit left, or one float"""
        n = self._tword_n.get(tid, 0)
        return self._tb_row(tid)[:n] if n else self._tb[tid]

    def _xp(self, t):
        """planes of activation tensor t for this forward pass (split once, shared by all consumers)"""
        buf = self._xplanes[t.tid]
        if t.tid not in self._xp_valid:
            ops.split_planes(self.act[t.tid], self.batch * t.h * t.w, t.c, out=buf)
            self._xp_valid.add(t.tid)
        return buf

    def _filter_units(self):
        return filter(has_filter, self.units)

    def _refresh_wplanes(self):
        if self._wp_valid or self._wplanes is None:
            return
        if self._jobs_wp is None:   # one batched launch for the planes of every filter (pointers never change)
            self._jobs_wp = ops.BatchJobs("split", self.device)
            for u in self._filter_units():
                if u.planes_fwd:
                    self._jobs_wp.add_split(self.params.view(u.p_kernel.name), u.wp, u.cout, u.k * u.k * u.src.c)
        self._jobs_wp.run()
        self._wp_valid = True

    def _refresh_wTplanes(self):
        if self._wTp_valid or self._wplanes is None:
            return
        self._refresh_wplanes()   # bound donors of the transposed filters
        if self._jobs_wTp is None:
            self._jobs_wTp = ops.BatchJobs("split", self.device)
            for u in self._filter_units():
                if u.cpad:
                    self._jobs_wTp.add_split(u.wT_pad, u.wTp_pad, u.src.c, u.cpad)
                elif u.planes_dgrad:
                    self._jobs_wTp.add_split(u.wT, u.wTp, u.src.c, u.k * u.k * u.cout, bound_from=u.wp)
        self._jobs_wTp.run()
        self._wTp_valid = True

    def _refresh_wT(self):
        if self._wT_valid:
            return
        if self._jobs_wT is None:
            self._jobs_wT = ops.BatchJobs("transpose", self.device)
            for u in self._filter_units():
                if u.cpad:
                    self._jobs_wT.add_transpose(u.w_pad, u.wT_pad, u.cpad, 1, u.src.c)
                else:
                    self._jobs_wT.add_transpose(self.params.view(u.p_kernel.name), u.wT, u.cout, u.k * u.k, u.src.c)
        for u in self.units:
            if u.kind == "head" and u.cpad:
                tape.torch_op(lambda u=u: u.w_pad[:u.out.c * u.src.c].copy_(self.params.view(u.p_kernel.name).reshape(-1)))
        self._jobs_wT.run()
        self._wT_valid = True

    def _conv_fwd(self, u, bias, out, stats=None, absmax=None):
        """the forward convolution of a conv / head unit: from planes where the unit has them, else the exact fp32 kernel"""
        if u.planes_fwd:
            return ops.conv2d_fwd_planes(u.desc, self._xp(u.src), u.wp, bias, out=out, stats=stats, absmax=absmax,
                                         precision=self._precision)
        return ops.conv2d_fwd(u.desc, self.act[u.src.tid], self.params.view(u.p_kernel.name), bias, out=out, stats=stats,
                              absmax=absmax)

    def _tight_bound(self, u):
        """whether the conv epilogue records per-channel max|y| for the bound of the BatchNorm output (YOLO_BN_TIGHT_BOUND:
        0 never, 1 always, 2 = not for 1x1 layers). Without it bn_finalize takes |y - mean| <= sqrt(P var), sqrt(P) / (max / sigma)
        ~ 2^6 looser: the planes' absolute error floor moves from 2^-40 to 2^-34 of the bound (planes.hpp)."""
        m = self._bn_tight
        return m == 1 or (m == 2 and u.k != 1)

    def _bn_bufs(self, u):
        c = u.cout
        b = self._bn_f32[u.bn_f32_off:u.bn_f32_off + 4 * c]
        ns = ops.BN_STAT_SLOTS * 2 * c
        nr = (ops.BN_RED_SLOTS + 1) * 2 * c
        return (b[0:c], b[c:2 * c], b[2 * c:3 * c], b[3 * c:4 * c], self._bn_f64[u.bn_f64_off:u.bn_f64_off + ns],
                self._bn_f64[u.bn_red_off:u.bn_red_off + nr])

    def _fold_infer_scale(self, u, scale, shift):
        """the folded inference scale / shift of a conv + BN unit: made once per set of weights. True if it was made now"""
        if self._infer_scale_valid:
            return False
        ops.bn_fold_inference(u.cout, self.params.view(u.p_gamma.name), self.params.view(u.p_beta.name),
                              self.state.view(u.s_mean.name), self.state.view(u.s_var.name), scale, shift)
        return True

    # ---- inference through a captured HIP graph ------------------------------------------------------------
    def infer(self, x, precision="fp32"):
        """forward(x, training=False, precision=precision) replayed from a hipGraph: a batch-1 forward is ~230 launches of
        a few microseconds each, i.e. launch-bound when enqueued one by one. The graph is captured per (batch size,
        precision) after an eager pass (which also refreshes the filter planes and the folded BN scales) and dropped
        whenever the parameters change. Outputs are the network's persistent head buffers, as with forward()."""
        ops.precision_enum(precision)
        if not self._use_infer_graph:
            return self.forward(x, training=False, precision=precision)
        x = x.contiguous()
        N = x.shape[0]
        # one graph per (batch size, precision); the fp32 graphs keep their bare batch-size key
        key = N if precision == "fp32" else (N, precision)
        g = self._infer_graphs.get(key)
        if g is None:
            self.forward(x, training=False, precision=precision)   # eager: allocations, weight prep, lazy module init
            static_in = x.clone()
            self.forward(static_in, training=False, precision=precision)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = self.forward(static_in, training=False, precision=precision)
            g = self._infer_graphs[key] = (graph, static_in, outs)
        graph, static_in, outs = g
        static_in.copy_(x)
        graph.replay()
        return outs

    def before_param_write(self):
        """Call BEFORE writing `params` / `state` on the current stream: a training-mode forward may still be
        transposing / splitting the old parameters on the second stream (its events are normally consumed by the first
        planes convolution and by backward; a forward without backward leaves them pending)."""
        for ev in (self._wp_event, self._wT_event):
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
        self._wp_event = self._wT_event = None

    def mark_params_changed(self):
        self.before_param_write()
        self._infer_graphs = {}
        self._wT_valid = False
        self._wp_valid = False
        self._wTp_valid = False
        self._infer_scale_valid = False

    # ---- forward ------------------------------------------------------------------------
    def forward(self, x, training=False, stop_after=None, precision="fp32"):
        """x: float32 CUDA tensor [N,H,W,C]. Returns the list of head outputs (coarse -> fine).
        stop_after (benchmarks only: bench.py's Darknet-53 block): name of the unit behind which the pass ends; returns None.
        precision: "fp32" (three MFMA passes per planes convolution) or, inference only, "fp16" (one pass on the fp16-rounded
        operands; the stem and the convolutions without planes operands stay exact)."""
        ops.precision_enum(precision)
        if training and precision != "fp32":
            raise ValueError("forward(training=True) is fp32-grade only: precision='fp16' is an inference mode")
        if x.dtype != torch.float32 or not x.is_cuda:
            raise YoloHipError("forward expects a float32 CUDA tensor")
        x = x.contiguous()
        if tuple(x.shape[1:]) != (self.input.h, self.input.w, self.input.c):
            raise YoloHipError(f"input shape {tuple(x.shape[1:])} != model input "
                               f"{(self.input.h, self.input.w, self.input.c)}")
        self.allocate(x.shape[0])
        self.training = training
        self._precision = precision
        self.act[self.input.tid] = x
        self._xp_valid = set()
        self._tbound_set = set()
        self._tword_n = {}        # tensors whose recorded bound is (still) the words of a one-pass inference unit
        self._prepare_filters(training)
        ops.zero_bytes(self._aux)   # bounds / per-channel maxima of this pass
        if training:
            ops.zero_bytes(self._bn_f64[:self._bn_stats_total])
            self._infer_scale_valid = False  # moving statistics (and the shared scale/shift) change
            # captured inference graphs were recorded with the folded scale/shift valid (no bn_fold_inference
            # inside): a training-mode forward overwrites those buffers with batch statistics, so drop them
            self._infer_graphs = {}
        prev_name = None
        for u in self.units:
            if stop_after is not None and prev_name == stop_after:
                self.training = False   # an incomplete pass: backward() must not run on it
                return None
            prev_name = u.name
            if self._wp_event is not None and has_filter(u) and u.planes_fwd:
                tape.wait_event(torch.cuda.current_stream(), self._wp_event)
                self._wp_event = None
            fwd = getattr(self, "_fwd_" + u.kind, None)
            if fwd is None:
                raise YoloHipError(f"unknown unit kind {u.kind}")
            fwd(u, training)
        if not training:
            self._infer_scale_valid = True
        return [self.act[t.tid] for t in self.outputs]

    def _prepare_filters(self, training):
        """the filters' planes for this pass; in training, beside the stem, with what backward needs
        (a pending event of an earlier forward stays until a planes conv / a backward has waited for it)"""
        if training and self._overlap_wgrad and self._prep_beside and not (self._wp_valid and self._wT_valid and self._wTp_valid):
            # the filters' planes (needed by the first planes conv) and their transposed forms (needed by backward) are
            # made on the second stream while the stem runs: 0.45 ms of HBM-bound launches beside MFMA-bound ones
            if self._wgrad_stream is None:
                self._wgrad_stream = ops.concurrent_stream("wgrad", device=self.device)
            side = self._wgrad_stream
            tape.wait_stream(side, torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._refresh_wplanes()
                self._wp_event = tape.record_event(side)
                self._refresh_wT()
                self._refresh_wTplanes()
                self._wT_event = tape.record_event(side)
        else:
            self._refresh_wplanes()

    def _fwd_conv(self, u, training):
        bias = self.params.view(u.p_bias.name) if u.p_bias is not None else None
        if not u.bn:
            self._conv_fwd(u, bias, u.y)
            if u.act != ACT_LINEAR:
                ops.act_fwd(u.y, u.act, out=u.a)
            if u.residual is not None:
                raise YoloHipError("residual without BN is not used by any reference graph")
            return
        scale, shift, smean, sinv, stats, _ = self._bn_bufs(u)
        if u.cout % 4:
            # a channel count the BatchNorm kernels do not walk (darknet19's class convolution): the exact fp32 convolution and
            # the one-workgroup-per-channel BatchNorm of csrc/classify.hip, with the same convention for the bias as below
            if u.residual is not None:
                raise YoloHipError(f"{u.name}: a residual Add needs a channel count that is a multiple of 4")
            self._conv_fwd(u, None if training else bias, u.y)
            ops.bn_act_any_fwd(u.y, u.cout, self.params.view(u.p_gamma.name), self.params.view(u.p_beta.name),
                               self.state.view(u.s_mean.name), self.state.view(u.s_var.name), scale, shift, smean, sinv, u.act,
                               u.a, training, mean_offset=bias, unbiased=self.unbiased_moving_var)
            return
        if training:
            # a conv bias in front of BatchNormalization (YOLOv1.5 / v2) cancels in (y - mean): the convolution
            # runs WITHOUT it -- u.y, the statistics and the saved mean are those of the bias-free tensor, so a
            # large bias cannot eat the digits of var = E[y^2] - mean^2 -- and only the moving mean adds it back
            amax = u.amax if self._tight_bound(u) else None
            self._conv_fwd(u, None, u.y, stats, amax)
            ops.bn_finalize(stats, u.y.numel() // u.cout, u.cout, self.params.view(u.p_gamma.name),
                            self.params.view(u.p_beta.name), self.state.view(u.s_mean.name), self.state.view(u.s_var.name),
                            scale, shift, smean, sinv, unbiased=self.unbiased_moving_var, bound=u.bound, absmax=amax,
                            mean_offset=bias)
            if u.pool_fuse is not None:
                return self._fwd_bn_act_pool(u, scale, shift)
        elif self._fuse_infer and (self._fused_infer_unit(u, bias, scale, shift)
                                   or (self._infer_onepass and self._stem_infer_unit(u, bias, scale, shift))):
            return
        else:
            self._conv_fwd(u, bias, u.y, absmax=u.amax)
            self._fold_infer_scale(u, scale, shift)
            ops.bn_infer_bound(u.cout, scale, shift, u.amax, u.bound)
        self._fwd_bn_act(u, training, scale, shift)

    def _fwd_bn_act_pool(self, u, scale, shift):
        """BatchNorm apply + activation + the 2x2 pool behind it + the pooled tensor's planes in one launch; the
        unpooled activation is not written (its only reader would have been the pool)"""
        pu = u.pool_fuse
        ppl = self._xplanes.get(pu.out.tid) if pu.out.c % 16 == 0 else None
        ops.bn_act_maxpool2x2_fwd(u.y, u.cout, scale, shift, u.act, pu.argmax,
                                  out=pu.buf if (pu.f32_needed or ppl is None) else None, planes=ppl,
                                  bn_bound=u.bound, out_bound=self._tb[pu.out.tid])
        self._tbound_set.add(pu.out.tid)
        if ppl is not None:
            self._xp_valid.add(pu.out.tid)
        pu.fused_this_pass = True

    def _fwd_bn_act(self, u, training, scale, shift):
        """BatchNorm apply + activation (+ residual Add) of a conv + BN unit, and the planes of its result"""
        res = self.act[u.residual.tid] if u.residual is not None else None
        res_pl = None
        if (res is not None and training and self._res_from_planes and u.cout % 16 == 0
                and u.residual.tid in self._xp_valid and u.residual.tid in self._tbound_set):
            res_pl, res = self._xplanes[u.residual.tid], None   # (its fp32 copy may not have been written)
        # consumers that are planes-capable convs get their operand straight from this kernel; the scale
        # comes from the bound bn_finalize (training) / bn_infer_bound (inference) derived from the conv
        # epilogue's per-channel max|y|
        pl = self._xplanes.get(u.out.tid) if u.cout % 16 == 0 else None
        if u.residual is not None and u.residual.tid not in self._tbound_set:
            pl = None   # residual without a recorded bound: split its consumers' operand separately
        else:
            self._tbound_set.add(u.out.tid)
        ops.bn_act_fwd(u.y, u.cout, scale, shift, u.act, res, out=u.a, planes=pl,
                       want_out=not (training and pl is not None and not u.a_needed), bn_bound=u.bound,
                       residual_bound=self._tb_float(u.residual.tid) if res is not None else None,
                       out_bound=self._tb[u.out.tid], residual_planes=res_pl)
        if pl is not None:
            self._xp_valid.add(u.out.tid)

    def _fwd_head(self, u, training):
        bias, anchors = self.params.view(u.p_bias.name), self._anchors_dev.get(u.name)
        if not training and self._infer_small_fuse and self._fuse_infer and u.planes_fwd:
            ops.conv2d_fwd_head_unit(u.desc, self._xp(u.src), u.wp, bias, u.A, u.C, u.version, anchors, u.t, u.yact,
                                     precision=self._precision)
            return
        self._conv_fwd(u, bias, u.t)
        ops.head_act_fwd(u.t, u.A, u.C, u.version, anchors, out=u.yact)

    def _fwd_upsample(self, u, training):
        if not training and self._infer_small_fuse and self._concat_planes and u.out.tid in self._up_producer:
            u.concat_reads_through = True   # (the Concatenate behind it reads the half-size tensor itself)
            return
        ops.upsample2x_fwd(self.act[u.src.tid], u.buf, u.out.c, 0)

    def _fwd_concat(self, u, training):
        pl = self._xplanes.get(u.out.tid) if self._concat_planes else None
        slots = [self._bound_alias.get(s.tid, s.tid) for s in u.srcs]
        ups = [self._up_producer.get(s.tid) for s in u.srcs]
        ups = [p if (p is not None and p.concat_reads_through) else None for p in ups]
        for p in ups:
            if p is not None:
                p.concat_reads_through = False
        rows, chans = self.batch * u.out.h * u.out.w, [s.c for s in u.srcs]
        dst32 = u.buf if u.f32_needed else None
        if (pl is not None and len(u.srcs) <= 4 and all(sl in self._tbound_set for sl in slots)
                and all(s.c % 8 == 0 for s in u.srcs)):
            if any(p is not None for p in ups):
                ops.split_planes_concat_ex([self.act[p.src.tid] if p is not None else self.act[s.tid]
                                            for s, p in zip(u.srcs, ups)], chans, [self._tb_words(sl) for sl in slots],
                                           rows, pl, upsample=[p is not None for p in ups], hw=(u.out.h, u.out.w),
                                           dst32=dst32, out_bound=self._tb[u.out.tid])
            else:
                ops.split_planes_concat([self.act[s.tid] for s in u.srcs], chans, [self._tb_float(sl) for sl in slots],
                                        rows, pl, dst32=dst32, out_bound=self._tb[u.out.tid])
            self._xp_valid.add(u.out.tid)
            self._tbound_set.add(u.out.tid)
            return
        for p in ups:   # (this Concatenate cannot read through after all: make the upsampled tensors now)
            if p is not None:
                ops.upsample2x_fwd(self.act[p.src.tid], p.buf, p.out.c, 0)
        off = 0
        for s in u.srcs:
            ops.copy_channels_in(self.act[s.tid], s.c, u.buf, u.out.c, off)
            off += s.c

    def _fwd_maxpool(self, u, training):
        if getattr(u, "fused_this_pass", False):   # made by its producer's BatchNorm launch (pool_fuse)
            u.fused_this_pass = False
            return
        ops.maxpool_fwd(self.act[u.src.tid], u.k, u.stride, u.pad_t, u.pad_l, u.out.h, u.out.w, u.buf,
                        u.out.c, 0, u.argmax if training else None)

    def _fwd_space_to_depth(self, u, training):
        ops.space_to_depth2_fwd(self.act[u.src.tid], u.buf, u.out.c, 0)

    def _fwd_gap(self, u, training):
        ops.gap_fwd(self.act[u.src.tid], out=u.buf)   # (the fp32 form of its input: plan._plan_fp32_copies)

    def _fwd_dense_softmax(self, u, training):
        ops.dense_softmax_fwd(self.act[u.src.tid], self.params.view(u.p_kernel.name), self.params.view(u.p_bias.name),
                              logits=u.logits, p=u.buf)

    def _stem_infer_unit(self, u, bias, scale, shift):
        """The RGB stem's inference unit in one launch (yolo_stem_fwd_infer_unit): direct fp32 convolution, folded
        BatchNormalization + activation in registers, the planes of the next convolution written by the same kernel; the image's
        max|x| comes from yolo_absmax_words. Returns False for any other unit."""
        pl = self._xplanes.get(u.out.tid)
        if u.residual is not None or pl is None or u.src.tid != self.input.tid or not ops.stem_infer_supported(u.desc):
            return False
        xin, w = self.act[u.src.tid], self.params.view(u.p_kernel.name)
        if self._fold_infer_scale(u, scale, shift):
            if getattr(u, "stem_wt", None) is None:
                u.stem_wt = torch.empty(28 * 32, device=self.device, dtype=torch.float32)
            ops.stem_filter_prep(w, bias, u.stem_wt)
            ops.zero_bytes(u.pred)
            ops.conv_pred_bound(w, u.cout, 27, scale, shift, bias, u.pred)
        row = self._tb_row(self.input.tid)
        n_in = ops.absmax_words(xin, row)
        nw = ops.stem_fwd_infer_unit(u.desc, xin, u.stem_wt, _epilogue(u), scale, shift, u.pred, row[:n_in],
                                     u.a if u.a_needed else None, pl, self._tb_row(u.out.tid))
        self._tword_n[u.out.tid] = nw
        self._tbound_set.add(u.out.tid)
        self._xp_valid.add(u.out.tid)
        return True

    def _fused_infer_unit(self, u, bias, scale, shift):
        """Inference form of a conv-BN-activation(-Add) unit in two launches (include/yolo_hip.h, fused epilogue): the
        folded BatchNormalization, the activation and the residual Add run in the conv's epilogue, then ONE pass turns
        the result into the planes of the consumer convolutions (bound = the epilogue's per-channel max + the
        residual's bound). Returns False when the unit keeps the three-launch path (no planes operand / consumer)."""
        if not u.planes_fwd or u.cout % 16 != 0:
            return False
        pl = self._xplanes.get(u.out.tid)
        own_planes = pl is not None
        if pl is None and self._infer_small_fuse and self._infer_onepass:
            # nobody reads this unit's result as planes (the FPN's lateral 1x1 conv in front of UpSampling2D): at few
            # output pixels the one-pass unit is still ONE launch where conv + reduce + bound + BatchNorm apply are four --
            # it writes planes of its own that nobody reads
            rows = self.batch * u.out.h * u.out.w
            if rows <= 4096:
                pl = self._xplanes_infer.get(u.out.tid)
                if pl is None:
                    pl = self._xplanes_infer[u.out.tid] = torch.zeros(ops.planes_bytes(rows, u.cout), device=self.device,
                                                                     dtype=torch.uint8)
        if pl is None or (u.residual is not None and u.residual.tid not in self._tbound_set):
            return False
        self._fold_infer_scale(u, scale, shift)
        res = self.act[u.residual.tid] if u.residual is not None else None
        src_slot = self._bound_alias.get(u.src.tid, u.src.tid)
        if self._infer_onepass and src_slot in self._tbound_set:
            # one pass: the kernel that finishes the tile writes the planes too, scaled by an a-priori bound
            if not self._infer_scale_valid:
                ops.zero_bytes(u.pred)
                ops.conv_pred_bound(self.params.view(u.p_kernel.name), u.cout, u.k * u.k * u.src.c, scale, shift, bias, u.pred)
            nw = ops.conv2d_fwd_infer_unit(u.desc, self._xp(u.src), u.wp, bias, _epilogue(u), scale, shift, res, u.a, u.amax,
                                           u.pred, self._tb_words(src_slot),
                                           self._tb_words(u.residual.tid) if u.residual is not None else None, pl,
                                           self._tb_row(u.out.tid), self._tb[u.out.tid], precision=self._precision)
            if nw:
                self._tword_n[u.out.tid] = nw
            self._tbound_set.add(u.out.tid)
            if own_planes:
                self._xp_valid.add(u.out.tid)
            return True
        if not own_planes:
            return False
        ops.conv2d_fwd_planes_epi(u.desc, self._xp(u.src), u.wp, bias, _epilogue(u), scale, shift, residual=res, out=u.a,
                                  absmax=u.amax, precision=self._precision)
        ops.split_planes_absmax(u.a, self.batch * u.out.h * u.out.w, u.cout, u.amax, pl,
                                extra_bound=self._tb_float(u.residual.tid) if u.residual is not None else None,
                                out_bound=self._tb[u.out.tid])
        self._tbound_set.add(u.out.tid)
        self._xp_valid.add(u.out.tid)
        return True

    # ---- backward -----------------------------------------------------------------------
    def _stem_fused_bwd(self, u):
        """the stem: BN / activation backward apply + filter gradient in one pass, no 32-channel dy tensor"""
        return (self._stem_fused and not (u.planes_wgrad or u.planes_dgrad) and not self._needs_grad[u.src.tid]
                and ops.stem_bn_bwd_supported(u.desc))

    def _takes_grad_slice(self, u):
        """can unit u's backward read dL/d(out) as a channel slice of a wider tensor? conv + BatchNormalization units without a
        residual Add (bn_act_bwd reads dout twice and nothing else does), not the fused stem path"""
        return u.kind == "conv" and u.bn and u.residual is None and u.cout % 8 == 0 and not self._stem_fused_bwd(u)

    def _add_grad(self, grads, t, buf):
        """Contribute `buf` (same shape as tensor t) to dL/dt: alias if first, else add in place."""
        if not self._needs_grad[t.tid]:
            return
        cur = grads.get(t.tid)
        if cur is None:
            grads[t.tid] = buf
        else:
            ops.axpy(cur, buf)

    def _grad_into(self, grads, t):
        """(the gradient buffer of source tensor t, whether to accumulate into it): what an earlier contributor left, or a
        new buffer, not initialised, that becomes dL/dt"""
        cur = grads.get(t.tid)
        if cur is not None:
            return cur, True
        cur = grads[t.tid] = torch.empty((self.batch, t.h, t.w, t.c), device=self.device, dtype=torch.float32)
        return cur, False

    def _gview(self, spec):
        return self.grads[spec.offset:spec.offset + spec.size]

    def backward(self, douts):
        """douts: list of dL/d(output) tensors (one per head, same order as forward's result).
        Parameter gradients are ACCUMULATED into self.grads (zeroed by the optimizer step)."""
        if not self.training:
            raise YoloHipError("backward() requires a preceding forward(training=True)")
        if self.backward_begin_hook is not None:
            tape.host_call(self.backward_begin_hook)
        if self._wT_event is not None:
            tape.wait_event(torch.cuda.current_stream(), self._wT_event)
            self._wT_event = None
        self._refresh_wT()
        self._refresh_wTplanes()
        for u in self.units:
            if getattr(u, "bnred", None) is not None:
                u.bnred_done = False
        grads = {t.tid: g for t, g in zip(self.outputs, douts)}
        for u in reversed(self.units):
            dout = grads.pop(u.out.tid, None)
            if dout is None:
                continue  # output unused by the loss
            if isinstance(dout, ops.ChannelSlice) and not self._takes_grad_slice(u):
                dout = dout.dense((self.batch, u.out.h, u.out.w, u.out.c))
            getattr(self, "_bwd_" + u.kind)(u, dout, grads)
            if self.grad_ready_hook is not None and plan.has_params(u):
                tape.host_call(lambda u=u: self.grad_ready_hook(u))
        self._join_wgrad()

    def _bwd_conv(self, u, dout, grads):
        if u.bn and u.cout % 4:   # (see _fwd_conv)
            scale, shift, smean, sinv, _, _ = self._bn_bufs(u)
            dy = ops.bn_act_any_bwd(u.y, dout, u.cout, self.params.view(u.p_gamma.name), scale, shift, smean, sinv, u.act,
                                    self._gview(u.p_gamma), self._gview(u.p_beta))
            return self._filter_and_data_grad(u, dy, self._dyp(u, dy), None, grads)
        if u.bn:
            scale, shift, smean, sinv, _, red = self._bn_bufs(u)
            if u.residual is not None:
                self._add_grad(grads, u.residual, dout)
            if self._stem_fused_bwd(u):
                ops.stem_bn_bwd_wgrad(u.desc, self.act[u.src.tid], u.y, dout, scale, shift, smean, sinv, u.act, red,
                                      self._gview(u.p_gamma), self._gview(u.p_beta), self._gview(u.p_kernel),
                                      fused=self._take_fused(u, dout))
                return
            # the gradient of the conv output goes straight into the planes the filter / data gradient
            # kernels read; the fp32 copy is written only if an fp32-path kernel still needs it
            # (a conv bias in front of BatchNormalization has the exact gradient 0 -- it cancels in y - mean -- so
            # nothing is computed for it: its slice of `grads` stays zero and no fp32 dy is needed on its account)
            need_f32 = (not u.planes_wgrad) or (self._needs_grad[u.src.tid] and not u.planes_dgrad)
            dyp = self._next_dyp_buffer(u) if (u.planes_wgrad or u.planes_dgrad) else None
            dy = ops.bn_act_bwd(u.y, dout, u.cout, self.params.view(u.p_gamma.name), scale, shift, smean,
                                sinv, u.act, red, self._gview(u.p_gamma), self._gview(u.p_beta),
                                planes=dyp, want_dx=need_f32, bound_aux=u.red_bound, fused=self._take_fused(u, dout),
                                tickets=u.tickets if self._bn_fold else None)
        else:
            dy = ops.act_bwd(u.y, dout, u.act) if u.act != ACT_LINEAR else dout
            dyp = self._dyp(u, dy)
        dbias = self._gview(u.p_bias) if (u.p_bias is not None and not u.bn) else None
        self._filter_and_data_grad(u, dy, dyp, dbias, grads)

    def _bwd_head(self, u, dout, grads):
        dt = ops.head_act_bwd(u.yact, dout, u.A, u.C, u.version, self._anchors_dev.get(u.name),
                              danchors=self._anchor_grad_views.get(u.name) if self.anchors_trainable else None)
        if not u.cpad:
            return self._filter_and_data_grad(u, dt, self._dyp(u, dt), self._gview(u.p_bias), grads)
        rows = self.batch * u.out.h * u.out.w
        dtp = ops.split_planes_padded(dt, rows, u.out.c, out=self._next_dyp_buffer(u))
        with self._beside_backward(dt):
            ops.zero_bytes(u.dw_pad)
            ops.conv2d_wgrad_planes(u.desc_pad, self._xplanes[u.src.tid], dtp, u.dw_pad)
            ops.axpy(self._gview(u.p_kernel), u.dw_pad[:u.out.c * u.src.c])
            ops.conv2d_wgrad_bias(dt, rows, u.out.c, self._gview(u.p_bias))
        if self._needs_grad[u.src.tid]:
            had = grads.get(u.src.tid)
            b = self._bnred_of(u, had)
            cur, acc = self._grad_into(grads, u.src)
            ops.conv2d_dgrad_planes(u.desc_pad, dtp, u.wTp_pad, dx=cur, accumulate=acc, bnred=b)

    def _filter_and_data_grad(self, u, dy, dyp, dbias, grads):
        """filter gradient of a conv / head unit beside the main stream, then its data gradient"""
        with self._beside_backward(dy):
            if u.planes_wgrad:
                ops.conv2d_wgrad_planes(u.desc, self._xplanes[u.src.tid], dyp, self._gview(u.p_kernel), dy=dy, dbias=dbias)
            else:
                ops.conv2d_wgrad(u.desc, self.act[u.src.tid], dy, self._gview(u.p_kernel), dbias)
        if not self._needs_grad[u.src.tid]:
            return
        b = self._bnred_of(u, grads.get(u.src.tid)) if u.planes_dgrad else None
        cur, acc = self._grad_into(grads, u.src)
        if u.planes_dgrad:
            ops.conv2d_dgrad_planes(u.desc, dyp, u.wTp, dx=cur, accumulate=acc, bnred=b)
        else:
            ops.conv2d_dgrad(u.desc, dy, u.wT, dx=cur, accumulate=acc)

    def _bwd_upsample(self, u, dout, grads):
        if self._needs_grad[u.src.tid]:
            cur, acc = self._grad_into(grads, u.src)
            ops.upsample2x_bwd(dout, u.out.c, 0, cur, accumulate=acc)

    def _bwd_concat(self, u, dout, grads):
        off = 0
        for s in u.srcs:
            if not self._needs_grad[s.tid]:
                pass
            elif (s.tid not in grads and self._concat_grad_slices and self._n_consumers.get(s.tid, 0) == 1
                    and s.producer is not None and self._takes_grad_slice(s.producer)
                    and s.c % 8 == 0 and off % 4 == 0 and u.out.c % 4 == 0):
                grads[s.tid] = ops.ChannelSlice(dout, u.out.c, off, s.c)   # read in place by bn_act_bwd
            else:
                cur, acc = self._grad_into(grads, s)
                ops.copy_channels_out(dout, u.out.c, off, cur, s.c, accumulate=acc)
            off += s.c

    def _bwd_maxpool(self, u, dout, grads):
        if not self._needs_grad[u.src.tid]:
            return
        N, had = self.batch, grads.get(u.src.tid)
        tiles = (u.k == 2 and u.stride == 2 and u.pad_t == 0 and u.pad_l == 0 and u.src.h == 2 * u.out.h
                 and u.src.w == 2 * u.out.w and u.out.c % 4 == 0 and torch.is_tensor(dout) and dout.is_contiguous()
                 and (had is None or torch.is_tensor(had)))
        cur, acc = self._grad_into(grads, u.src)
        if tiles:
            # the windows tile the input: every input position is written / added to once, no zero fill, no atomics
            ops.maxpool2x2_bwd(dout, N, u.out.h, u.out.w, u.out.c, u.argmax, cur, acc)
            return
        if not acc:
            ops.zero_bytes(cur)
        if u.stride == 1 and (u.out.h, u.out.w) == (u.src.h, u.src.w):
            ops.maxpool_bwd_same(dout, N, u.out.h, u.out.w, u.out.c, u.out.c, 0, u.argmax, u.k, u.pad_t, u.pad_l, cur)
        else:
            ops.maxpool_bwd(dout, N, u.out.h, u.out.w, u.out.c, u.out.c, 0, u.argmax, cur)

    def _bwd_gap(self, u, dout, grads):
        if not self._needs_grad[u.src.tid]:
            return
        cur = grads.get(u.src.tid)
        if cur is None:
            grads[u.src.tid] = ops.gap_bwd(dout, u.dsrc, accumulate=False)
        else:
            ops.gap_bwd(dout, cur, accumulate=True)

    def _fwd_softmax(self, u, training):
        ops.dense_softmax_fwd(self.act[u.src.tid], None, None, p=u.buf)

    def _bwd_softmax(self, u, dout, grads):
        if self._needs_grad[u.src.tid]:
            ops.dense_softmax_bwd(dout, u.buf, None, None, u.dsrc)
            self._add_grad(grads, u.src, u.dsrc)

    def _bwd_dense_softmax(self, u, dout, grads):
        ops.dense_softmax_bwd(dout, u.buf, self.act[u.src.tid], self.params.view(u.p_kernel.name), u.dsrc,
                              dw=self._gview(u.p_kernel), db=self._gview(u.p_bias), dz=u.dz)
        self._add_grad(grads, u.src, u.dsrc)

    def _bwd_space_to_depth(self, u, dout, grads):
        if self._needs_grad[u.src.tid]:
            cur, acc = self._grad_into(grads, u.src)
            ops.space_to_depth2_bwd(dout, u.out.c, 0, cur, accumulate=acc)

    # The filter gradient of a layer is independent of everything the backward pass does next (its data
    # gradient, the BatchNorm backward of the layer below, ...): it is enqueued on a second stream so that it
    # shares the chip with them -- the conv kernels alone leave workgroup slots idle in their last round (344
    # or 676 tiles on 512 slots) and the BatchNorm kernels leave the matrix pipe idle. Hazards: the dy planes
    # scratch is double-buffered and re-used only after the filter gradient that read it has finished (event);
    # fp32 tensors read on the second stream are marked with record_stream; the main stream joins the second
    # one at the end of backward. A grad_ready_hook (data parallel gradient buckets) must order its work after
    # BOTH streams (dp.GradReducer.extra_streams).
    def _next_dyp_buffer(self, u=None):
        if u is not None and u.name in self._dyp_own:
            self._dyp_cur_own = True
            return self._dyp_own[u.name]
        self._dyp_cur_own = False
        self._dyp_idx ^= 1
        ev = self._dyp_events[self._dyp_idx]
        if ev is not None:
            tape.wait_event(torch.cuda.current_stream(), ev)
            self._dyp_events[self._dyp_idx] = None
        if self._dyplanes2[self._dyp_idx] is None and self._dyp_shared_bytes:
            self._dyplanes2[self._dyp_idx] = torch.empty(self._dyp_shared_bytes, device=self.device, dtype=torch.uint8)
        return self._dyplanes2[self._dyp_idx]

    @contextlib.contextmanager
    def _beside_backward(self, *tensors):
        if not self._overlap_wgrad:
            yield
            return
        if self._wgrad_stream is None:
            self._wgrad_stream = ops.concurrent_stream("wgrad", device=self.device)
        side = self._wgrad_stream
        tape.wait_stream(side, torch.cuda.current_stream())
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        with torch.cuda.stream(side):
            yield
            # (the event guards the REUSE of a shared dy planes buffer: a layer with planes of its own needs none)
            ev = None if getattr(self, "_dyp_cur_own", False) else tape.record_event(side)
        if ev is not None:
            self._dyp_events[self._dyp_idx] = ev
        self._wgrad_pending = True

    def _join_wgrad(self):
        if self._wgrad_pending:
            tape.wait_stream(torch.cuda.current_stream(), self._wgrad_stream)
            self._wgrad_pending = False

    def _dyp(self, u, dy):
        """planes of this layer's dy (one scratch, consumed by the filter and data gradients right away)"""
        if not (u.planes_wgrad or u.planes_dgrad):
            return None
        return ops.split_planes(dy, self.batch * u.out.h * u.out.w, u.cout, out=self._next_dyp_buffer(u))

    def _bnred_of(self, w, cur):
        """the fused reduction this writer's data gradient makes (None: none). cur = the gradient it adds into, if any: a
        ChannelSlice or a tensor that is not dense NHWC of the source never takes the fused form"""
        p = w.bnred_for
        if p is None or p.bnred is None or (cur is not None and not torch.is_tensor(cur)):
            return None
        p.bnred_done = True
        return p.bnred

    def _take_fused(self, u, dout):
        """the BnReduce that already holds the reduction of `dout` for unit u's BatchNormalization backward, or None"""
        b = getattr(u, "bnred", None)
        if b is None or not u.bnred_done:
            return None
        u.bnred_done = False
        if not torch.is_tensor(dout):
            raise YoloHipError(f"{u.name}: fused reduction made for a gradient that arrives as a channel slice")
        return b

    # ---- weights ------------------------------------------------------------------------
    def named_weights(self):
        """name -> numpy array in KERAS layout (kernel HWIO), for .npz interchange."""
        out = {}
        for store in (self.params, self.state):
            for name in store.order:
                s = store.specs[name]
                a = store.view(name).detach().cpu().numpy().reshape(s.shape)
                if name.endswith("/kernel"):
                    a = np.transpose(a, (1, 2, 3, 0) if a.ndim == 4 else (1, 0))  # KRSC -> HWIO, Dense [K,C] -> [C,K]
                out[name] = a.copy()
        return out

    def load_named_weights(self, weights, strict=True):
        self.before_param_write()
        for store in (self.params, self.state):
            for name in store.order:
                if name not in weights:
                    if strict:
                        raise KeyError(f"missing weight {name}")
                    continue
                s = store.specs[name]
                a = np.asarray(weights[name], dtype=np.float32)
                if name.endswith("/kernel"):
                    a = np.transpose(a, (3, 0, 1, 2) if a.ndim == 4 else (1, 0))  # HWIO -> KRSC, Dense [C,K] -> [K,C]
                if tuple(a.shape) != s.shape:
                    raise ValueError(f"{name}: shape {a.shape} != {s.shape}")
                store.view(name).copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        self.mark_params_changed()
