"""The static plan of the executor (engine.Network): every decision about a built graph that needs no device.

  * `Options.from_env()`: the YOLO_* switches of the executor, read once per Network;
  * `plan_graph`: what does not depend on the batch size -- which units run on planes and where their filter planes live,
    head padding, which fp32 activations are never written, pool fusion, bound aliases, read-through upsampling, the
    layouts of the flat buffers, the fused-reduction writers. Per-unit results are attributes on the units; graph-level
    results (needs_grad, consumers, n_consumers, bound_alias, up_producer, the *_total sizes) come back in one namespace;
  * `plan_batch`: what `Network.allocate` derives from the batch size -- conv descriptors, pool pads, planes sizes, the
    BatchNormalization-backward reductions made by data gradients.

Pure host code: it asks the library host-side questions through `ops` (planes_bytes, bnred_slots_cap, conv_desc, the *_ok
predicates) and touches no device, so tests/test_plan_cpu.py checks all of it without one."""
import os
from types import SimpleNamespace

from . import ops

# words of the bounds / tickets block of a unit in Network._aux (zeroed at the start of every forward pass): [0] bound of the
# BatchNorm output, [1..68] the 68 words of yolo_bn_act_bwd_reduce_bound, [69..104] ticket words of its in-launch fold;
# a conv + BN unit has its per-channel max|conv out| (conv epilogue) behind them: [AUX_WORDS .. +C)
AUX_WORDS = 112


class Options:
    """the executor's environment switches; read when a Network is constructed"""

    @classmethod
    def from_env(cls, env=None):
        env = os.environ if env is None else env
        o = cls()

        def on(name):
            return env.get(name, "1") != "0"
        o.overlap_wgrad = on("YOLO_BWD_OVERLAP")      # filter gradients on a second stream (engine: _beside_backward)
        o.prep_beside = on("YOLO_PREP_OVERLAP")       # filter preparation beside the stem
        o.stem_fused = on("YOLO_STEM_FUSED_BWD")      # stem: BN backward apply + wgrad in one pass
        o.bn_tight = int(env.get("YOLO_BN_TIGHT_BOUND", "0"))   # engine: _tight_bound
        o.res_from_planes = on("YOLO_RES_PLANES")     # residual adds read the planes, not an fp32 copy
        o.use_infer_graph = on("YOLO_INFER_GRAPH")
        o.fuse_infer = on("YOLO_INFER_FUSE")
        # the gradient of a Concatenate reaches the BatchNormalization backward of its sources as a channel SLICE of the
        # concat's gradient (ops.ChannelSlice: read in place with its row pitch) instead of being copied out per source
        o.concat_grad_slices = on("YOLO_CONCAT_GRAD_SLICE")
        # YOLO_DYP_PER_LAYER=1 (default): every layer has its OWN dy planes instead of two shared ones -- 288 GB of HBM make
        # the reuse pointless (YOLOv3-416 at bs 32: +4.6 GB), and the reuse costs the compute stream a wait on the
        # filter-gradient stream's event per layer: a barrier packet in its queue even when the event has long fired (2.4 us
        # each, 75 per step, measured with scripts/hip_probe/event_gap_probe.cpp: profiles/r05_a_event_gap_probe.log) plus
        # the event record on the side stream. Across steps the buffers are safe: backward joins the filter-gradient stream
        # before it returns.
        o.dyp_per_layer = on("YOLO_DYP_PER_LAYER")
        # YOLO_BN_FOLD=1 finishes the BatchNormalization-backward reduction inside its own launch
        # (yolo_bn_act_bwd_reduce_fold_ld: the last workgroups to arrive fold the slots) instead of a bn_bwd_sum launch per
        # layer: 72 launches fewer. Default 0: measured neutral on YOLOv3-416 (28.99 / 28.99 ms) and 1 % SLOWER on YOLOv4-608
        # (37.20 -> 37.56: profiles/r06_a_bn_fold_ab_*.log) -- the two dependent memory-side round trips of the fold's tail
        # cost what the 8 us launch cost behind a queue that dispatches back to back
        o.bn_fold = env.get("YOLO_BN_FOLD", "0") == "1"
        # The BatchNormalization-backward reduction of a conv + BN unit P (sums of dz and dz * xhat over dL/d(P.out)) is made
        # by the data gradient that COMPLETES dL/d(P.out) -- the last contribution in backward order, when that is a planes
        # data gradient (include/yolo_hip.h: yolo_conv2d_dgrad_planes_bnred): W.bnred_for = P on that writer W.
        # YOLO_BN_FUSED_REDUCE: 0 never, 1 every planes data gradient that completes a tensor, or a set of writer classes
        # "w" (3x3 stride-1 with enough tiles to run unsplit), "s" (stride 2), "p" (1x1), "h" (heads), "t" (the small
        # 3x3 layers that lose their split-K), e.g. "ws"
        # Default 0: measured (profiles/r05_a_*): the step does not get shorter with it -- the y tile costs the data gradient as
        # much as the standalone pass cost beside the filter-gradient stream.
        o.bn_fused_reduce = env.get("YOLO_BN_FUSED_REDUCE", "0")
        # heads whose channel count is not a multiple of 16 (YOLOv3: 255): the backward kernels run on the channel count
        # rounded up to 16 - head gradient planes with zero columns, filters with zero rows
        o.head_pad = on("YOLO_HEAD_PAD")
        # conv + BN + activation units whose ONLY consumer is a 2x2 / stride-2 pool that tiles their output (Darknet-19,
        # tiny-YOLOv3): in training the BatchNorm apply, the pool and the planes of the pooled tensor are ONE launch
        # (yolo_bn_act_maxpool2x2_fwd) and the unpooled activation is never written (YOLO_POOL_FUSE=0: three launches)
        o.pool_fuse = on("YOLO_POOL_FUSE")
        # concat units write the planes of their result directly from the fp32 sources (yolo_split_planes_concat): the fp32
        # concatenation is produced only if somebody other than a planes convolution reads it
        o.concat_planes = on("YOLO_CONCAT_PLANES")
        o.infer_onepass = on("YOLO_INFER_ONEPASS")
        # bs-1 predict (no launch of the replayed graph costs less than ~4.5 us: DESIGN.md section 3.10):
        # (a) an UpSampling2D(2) whose only reader is a Concatenate is read THROUGH by the concat's planes pass (inference),
        # which also takes the sources' bounds as the words the one-pass units left instead of a fold launch per source
        # (yolo_split_planes_concat_ex); (b) a conv + BN unit nobody reads as planes (the FPN's lateral 1x1 in front of the
        # upsampling) still runs as a one-pass unit into planes of its own that nobody reads -- one launch instead of four;
        # (c) the heads: convolution + activation in one call (yolo_conv2d_fwd_head_unit). YOLO_INFER_SMALL_FUSE=0: off
        o.infer_small_fuse = on("YOLO_INFER_SMALL_FUSE")
        # stride 2: the four parity classes of the data gradient are ONE launch (csrc/conv.hip: dgrad_impl)
        o.dgrad_classes = on("YOLO_DGRAD_CLASSES")
        return o


def has_filter(u):
    return u.kind in ("conv", "head")


def has_params(u):
    """units that own a slice of the flat parameter / gradient buffers"""
    return u.kind in ("conv", "head", "dense_softmax")


def reads_as_planes(c, t):
    """consumer c takes tensor t as the planes operand of its forward convolution and of its filter gradient, and in no
    other way: it never reads an fp32 copy of t"""
    return has_filter(c) and c.src.tid == t.tid and c.residual is not t and c.planes_fwd and c.planes_wgrad


def _fp32_read(t, g, also=lambda c: False):
    """whether anybody reads the fp32 form of tensor t: the caller (a network output), nobody at all (then the fp32 form
    is all there is), or a consumer that neither reads_as_planes nor satisfies `also`"""
    cs = g.consumers.get(t.tid, [])
    return t.tid in g.out_tids or not cs or any(not (reads_as_planes(c, t) or also(c)) for c in cs)


def plan_graph(units, tensors, input, outputs, opts):
    """everything that does not depend on the batch size; per-unit results are set on the units"""
    g = SimpleNamespace(out_tids={t.tid for t in outputs})
    # consumers per tensor decide whether a tensor needs a gradient at all
    g.needs_grad = {input.tid: False}
    for u in units:
        g.needs_grad[u.out.tid] = has_params(u) or any(g.needs_grad[t.tid] for t in u.inputs)
    g.consumers, g.n_consumers = {}, {}
    for u in units:
        for t in u.inputs:
            g.consumers.setdefault(t.tid, []).append(u)
            g.n_consumers[t.tid] = g.n_consumers.get(t.tid, 0) + 1
    for t in outputs:
        g.n_consumers[t.tid] = g.n_consumers.get(t.tid, 0) + 1
    _plan_param_buffers(g, units)
    _plan_fused_reduce(g, units, tensors, opts)
    _plan_filter_planes(g, units, opts)
    _plan_fp32_copies(g, units, opts)
    _plan_bounds(g, units, tensors)
    return g


def _plan_param_buffers(g, units):
    """layouts of _wT (transposed filters), _bn_f32 and _bn_f64"""
    wT = f32 = f64 = 0
    for u in units:
        if u.kind == "conv" and u.bn:
            u.bn_f32_off = f32
            f32 += 4 * u.cout            # scale, shift, save_mean, save_invstd
            u.bn_f64_off = f64           # stats[SLOTS][2C]; all layers' statistics are contiguous: they are
            f64 += ops.BN_STAT_SLOTS * 2 * u.cout   # the part of the fp64 buffer that is zeroed every step
        if has_filter(u):
            u.wT_off = wT
            wT += u.cout * u.k * u.k * u.src.c
    g.bn_stats_total = f64
    for u in units:              # red[RED_SLOTS+1][2C]: every slot is written before it is read, never zeroed
        if u.kind == "conv" and u.bn:
            u.bn_red_off = f64
            f64 += (ops.BN_RED_SLOTS + 1) * 2 * u.cout
    g.wT_total, g.bn_f32_total, g.bn_f64_total = wT, f32, f64


def _plan_fused_reduce(g, units, tensors, opts):
    """static walk of backward(): who contributes to dL/d(tensor), in which order. The last contributor of a tensor
    produced by a conv + BatchNormalization unit P gets W.bnred_for = P if it is a conv / head unit (whether its data
    gradient is a planes kernel is known later: plan_batch checks). A skipped writer (its own gradient never arrives) simply
    never sets the flag P's backward looks for, and P makes the reduction itself."""
    last = {}
    for u in reversed(units):
        u.bnred_for = None
        if u.kind == "conv" and u.bn and u.residual is not None and g.needs_grad[u.residual.tid]:
            last[u.residual.tid] = ("add", u)
        if has_filter(u):
            if g.needs_grad[u.src.tid]:
                last[u.src.tid] = ("dgrad", u)
        else:
            for t in u.inputs:
                if g.needs_grad[t.tid]:
                    last[t.tid] = ("other", u)
    mode = opts.bn_fused_reduce
    if mode == "0":
        return
    for tid, (how, w) in last.items():
        p = tensors[tid].producer
        if how != "dgrad":
            continue
        # (stride 2: the four parity classes of the data gradient must be ONE launch, csrc/conv.hip: dgrad_impl)
        one_launch = w.stride == 1 or (w.stride == 2 and w.k == 3 and opts.dgrad_classes)
        if not (one_launch and p is not None and p.kind == "conv" and p.bn and p.cout % 4 == 0):
            continue
        if w.kind == "head":
            cls = "h"
        elif w.stride == 2:
            cls = "s"
        elif w.k == 1:
            cls = "p"
        else:
            cls = "w"
        w.bnred_class = cls
        if mode == "1" or cls in mode or (cls == "w" and "t" in mode):
            w.bnred_for = p


def _plan_filter_planes(g, units, opts):
    """pre-split ("planes") copies of the filters for the LDS-DMA conv kernels: [Cout][taps*Cin] for forward,
    [Cin][taps*Cout] for dgrad, regions of ONE buffer (_wplanes) at 256-byte boundaries"""
    total = 0

    def region(nbytes):
        nonlocal total
        off = total
        total += (nbytes + 255) // 256 * 256
        return off, nbytes
    for u in filter(has_filter, units):
        cin, taps = u.src.c, u.k * u.k
        u.planes_fwd = ops.planes_fwd_ok(cin, u.cout)
        u.planes_dgrad = ops.planes_dgrad_ok(cin, u.cout) and g.needs_grad[u.src.tid]
        u.planes_wgrad = u.planes_fwd and ops.planes_wgrad_ok(cin, u.cout, taps, u.stride)
        u.wp_off = u.wTp_off = -1
        u.cpad = 0   # (Options.head_pad)
        if u.kind == "head" and u.cout % 16 != 0 and not u.planes_dgrad and opts.head_pad:
            cp = (u.cout + 15) // 16 * 16
            if u.planes_fwd and ops.planes_wgrad_ok(cin, cp, 1) and ops.planes_dgrad_ok(cin, cp):
                u.cpad = cp
                u.wTp_pad_off, u.wTp_pad_bytes = region(ops.planes_bytes(cin, cp))
        if u.planes_fwd:
            u.wp_off, u.wp_bytes = region(ops.planes_bytes(u.cout, taps * cin))
        if u.planes_dgrad:
            u.wTp_off, u.wTp_bytes = region(ops.planes_bytes(cin, taps * u.cout))
    g.wplanes_total = total


def _plan_fp32_copies(g, units, opts):
    """which fp32 activations are never written in training (a_needed, f32_needed, pool_fuse), whose bound a tensor
    shares (bound_alias), which upsamplings a Concatenate reads through (up_producer)"""
    for u in units:
        u.pool_fuse = None
        if u.kind != "conv":
            continue
        # the fp32 copy of a conv unit's output is written in training only if somebody reads it: consumers that take
        # it as a planes operand (planes conv / head units) do not, nor do conv + BN units that ADD it as their
        # residual (bn_act_fwd reads the residual from the planes too, yolo_bn_act_fwd_res_planes)
        def adds_from_planes(c, t=u.out):
            return (opts.res_from_planes and c.kind == "conv" and c.bn and c.residual is t and c.src.tid != t.tid
                    and c.cout % 16 == 0)
        cs = g.consumers.get(u.out.tid, [])
        has_planes_src = any(has_filter(c) and c.src.tid == u.out.tid and c.planes_fwd for c in cs)
        u.a_needed = u.cout % 16 != 0 or not has_planes_src or _fp32_read(u.out, g, also=adds_from_planes)
        # (Options.pool_fuse)
        if not opts.pool_fuse or not u.bn or u.residual is not None or u.out.tid in g.out_tids:
            continue
        if len(cs) != 1 or cs[0].kind != "maxpool":
            continue
        p = cs[0]
        if (p.k == 2 and p.stride == 2 and u.out.h % 2 == 0 and u.out.w % 2 == 0 and p.out.h * 2 == u.out.h
                and p.out.w * 2 == u.out.w and u.cout % 8 == 0 and p.padding in ("same", "valid")):
            p.f32_needed = p.out.c % 16 != 0 or _fp32_read(p.out, g)
            u.pool_fuse = p
    # (Options.concat_planes) a source's bound is the one its producer recorded -- BatchNorm's output bound, or, through
    # pools / upsampling / space-to-depth (which cannot increase max|x|), their input's
    g.bound_alias, g.up_producer = {}, {}
    for u in units:
        if u.kind in ("upsample", "maxpool", "space_to_depth"):
            g.bound_alias[u.out.tid] = g.bound_alias.get(u.src.tid, u.src.tid)
        elif u.kind == "concat":
            u.f32_needed = _fp32_read(u.out, g)
        # (Options.infer_small_fuse, a)
        if u.kind == "upsample" and g.n_consumers.get(u.out.tid, 0) == 1 and u.out.tid not in g.out_tids:
            cs = g.consumers.get(u.out.tid, [])
            if (len(cs) == 1 and cs[0].kind == "concat" and u.out.h == 2 * u.src.h and u.out.w == 2 * u.src.w
                    and u.out.c == u.src.c):
                g.up_producer[u.out.tid] = u


def _plan_bounds(g, units, tensors):
    """bounds for the planes scales (planes.hpp) in _aux: AUX_WORDS per unit (+ the per-channel maxima of a conv + BN
    unit), zeroed every step, and one float per tensor = bound of that activation. The per-tensor bounds live behind the
    units' words: zeroed with them at the start of every forward pass, which the one-pass inference units need -- their
    kernels raise the bound of their result with atomicMax.
    _pred: {K, D} of every conv-BN unit for the a-priori bound of its inference output (ops.conv_pred_bound): made with the
    folded scale / shift, i.e. once per set of weights"""
    off = 0
    for i, u in enumerate(units):
        u.aux_off = off
        off += AUX_WORDS
        if u.kind == "conv" and u.bn:
            off += (u.cout + 7) // 8 * 8
        u.pred_off = 2 * i
    g.tbound_off = max(off, 1)
    g.aux_total = g.tbound_off + max(len(tensors), 1) + 1
    g.pred_total = 2 * max(len(units), 1)


def plan_batch(units, N, opts):
    """what Network.allocate derives from the batch size N: conv descriptors (desc, desc_pad) and pool pads by unit name,
    the bytes of each activation's planes by tensor id, of each unit's own dy planes and of one buffer of the shared pair,
    and the slot capacity of every BnReduce by the name of the unit whose reduction it is"""
    b = SimpleNamespace(desc={}, desc_pad={}, pool_pad={}, xplanes_bytes={}, dyp_own_bytes={}, dyp_shared_bytes=0,
                        bnred_cap={})
    for u in units:
        if u.kind == "maxpool":
            same = u.padding == "same"
            b.pool_pad[u.name] = (ops.same_pad(u.src.h, u.k, u.stride)[1] if same else 0,
                                  ops.same_pad(u.src.w, u.k, u.stride)[1] if same else 0)
        if not has_filter(u):
            continue
        shape = (N, u.src.h, u.src.w, u.src.c)
        b.desc[u.name] = ops.conv_desc(shape, u.cout, u.k, u.k, u.stride, u.padding)
        # planes of the activations that feed planes-capable convs (kept from forward for the filter gradient)
        if u.planes_fwd and u.src.tid not in b.xplanes_bytes:
            b.xplanes_bytes[u.src.tid] = ops.planes_bytes(N * u.src.h * u.src.w, u.src.c)
        # planes of the layer's dy in backward: its own buffer (Options.dyp_per_layer) or the shared pair
        if u.cpad:
            b.desc_pad[u.name] = ops.conv_desc(shape, u.cpad, 1, 1, 1, "same")
        elif not (u.planes_dgrad or u.planes_wgrad):
            continue
        nb = ops.planes_bytes(N * u.out.h * u.out.w, u.cpad or u.cout)
        b.dyp_shared_bytes = max(b.dyp_shared_bytes, nb)
        if opts.dyp_per_layer:
            b.dyp_own_bytes[u.name] = nb
    # slots of the BatchNormalization-backward reductions made by data gradients (_plan_fused_reduce)
    for w in units:
        p = w.bnred_for
        if p is None or not (w.planes_dgrad or w.cpad):
            continue
        if getattr(w, "bnred_class", "") == "w" and opts.bn_fused_reduce != "1":
            # 3x3 stride-1 launches of at most 256 tiles run split-K (csrc/conv_win.hip: conv_split_parts), which the
            # fused form gives up: their own class "t"
            small = -(-N * w.src.h * w.src.w // 128) * -(-w.src.c // 128) <= 256
            if ("t" if small else "w") not in opts.bn_fused_reduce:
                continue
        cap = ops.bnred_slots_cap(b.desc[w.name])   # (a head with padded channels uses desc_pad: same pixels, same Cin)
        if cap > 0:
            b.bnred_cap[p.name] = cap
    return b
