"""The streaming glue kernels (csrc/elementwise.hip, the C % 8 == 4 and stand-alone activation kernels of csrc/bn_act.hip,
csrc/labels.hip, csrc/iou.hip) PAST THEIR GRID CAP and at the edges of their channel slices.

stream_grid() stops at 2048 workgroups of 256 threads; beyond 524 288 work items a thread reaches its next item through
`i += gridDim.x * blockDim.x`. Every "past the cap" case of tests/past_cap_cases.py has its work items in (2 cap, 3 cap]
and no multiple of the cap: a first, a middle and a partial last pass. References are torch on the CPU: float64 for
anything with arithmetic (oracle/layers.py), plain indexing for data movement. Pure data movement must be BIT-equal;
arithmetic is held to TOL = 1e-4 PER ELEMENT relative to max(1, |ref|), so that one wrong element cannot hide behind a large
one. The launcher branches no other test reaches -- scalar channel copies, accumulate forms, c_off != 0, the general pool
into a slice, the fall-through of the 2x2 fast path, act_fwd / act_bwd, axpy, fill -- are run here at both sizes."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import past_cap_cases as PC
from oracle import layers as L

pytestmark = pytest.mark.gpu
TOL = 1e-4
SENT = -123.5          # sentinel of the elements a kernel must leave alone


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref, what=""):
    """|got - ref| <= TOL max(1, |ref|) in every element; returns the worst such ratio"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs() / ref.abs().clamp(min=1.0)
    worst = err.max().item()
    assert worst <= TOL, (what, worst, int(err.argmax()))
    return worst


def _same(got, ref, what=""):
    assert torch.equal(got.cpu(), ref), what


def _ties(g, shape):
    """small integers plus quarter steps: many exact ties inside a window, every value exact in fp32"""
    m = torch.randint(-6, 7, shape, generator=g).double()
    return m + 0.25 * torch.randn(shape, generator=g, dtype=torch.float64).round()


# ---- channel-slice copies ---------------------------------------------------------------------------------------------
def _copy_in(P, Csrc, Cdst, c_off, seed=1):
    from tf2_yolo_amd import ops
    src = torch.randn(P, Csrc, generator=_gen(seed))
    dst = torch.full((P, Cdst), SENT, device="cuda")
    ops.copy_channels_in(src.cuda(), Csrc, dst, Cdst, c_off)
    ref = torch.full((P, Cdst), SENT)
    ref[:, c_off:c_off + Csrc] = src
    _same(dst, ref, ("copy_in", P, Csrc, Cdst, c_off))       # the slice, and the sentinel everywhere else


def _copy_out(P, Csrc, Cdst, c_off, accumulate, seed=2):
    from tf2_yolo_amd import ops
    g = _gen(seed)
    src = torch.randn(P, Csrc, generator=g)
    dst0 = torch.randn(P, Cdst, generator=g)
    dst = dst0.cuda()
    srcd = src.cuda()
    ops.copy_channels_out(srcd, Csrc, c_off, dst, Cdst, accumulate=accumulate)
    sl = src[:, c_off:c_off + Cdst]
    _same(dst, dst0 + sl if accumulate else sl.contiguous(), ("copy_out", P, Csrc, Cdst, c_off, accumulate))
    _same(srcd, src)


@pytest.mark.parametrize("name", ["copy_in_vec", "copy_in_scalar"])
def test_copy_channels_in_past_the_cap(name):
    _copy_in(**PC.GLUE[name].d)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name", ["copy_out_vec", "copy_out_scalar"])
def test_copy_channels_out_past_the_cap(name, accumulate):
    """vectorised and scalar form, assign and accumulate (the engine's second consumer of a concat source), the slice at
    the start, in the middle and at the end of the source"""
    d = PC.GLUE[name].d
    assert d["c_offs"][0] == 0 and d["c_offs"][-1] + d["Cdst"] == d["Csrc"]
    for c_off in d["c_offs"]:
        _copy_out(d["P"], d["Csrc"], d["Cdst"], c_off, accumulate)


@pytest.mark.parametrize("P,Csrc,Cdst,c_off", [(1, 4, 4, 0), (1, 4, 12, 8), (37, 4, 8, 4), (1, 1, 1, 0), (37, 1, 3, 2),
                                               (37, 2, 7, 5), (37, 5, 9, 0), (37, 4, 9, 4), (37, 4, 8, 2), (300, 8, 20, 12)])
def test_copy_channels_small_edges(P, Csrc, Cdst, c_off):
    """C = 4 (the narrowest vector form), C = 1 / 2 / 5, one pixel; a vector-sized slice that is scalar only because the
    wide tensor (Cdst = 9) or the offset (c_off = 2) is no multiple of 4"""
    _copy_in(P, Csrc, Cdst, c_off)
    for acc in (False, True):
        _copy_out(P, Cdst, Csrc, c_off, acc)


# ---- nearest 2x up-sampling -------------------------------------------------------------------------------------------
def _upsample_fwd(N, H, W, C, Cy, c_off, seed=3):
    from tf2_yolo_amd import ops
    x = torch.randn(N, H, W, C, generator=_gen(seed))
    y = torch.full((N, 2 * H, 2 * W, Cy), SENT, device="cuda")
    ops.upsample2x_fwd(x.cuda(), y, Cy, c_off)
    ref = torch.full((N, 2 * H, 2 * W, Cy), SENT)
    ref[..., c_off:c_off + C] = L.upsample2x(x)
    _same(y, ref, ("upsample_fwd", N, H, W, C, Cy, c_off))


def _upsample_bwd(N, H, W, C, Cy, c_off, seed=4):
    from tf2_yolo_amd import ops
    g = _gen(seed)
    dy = torch.randn(N, 2 * H, 2 * W, Cy, generator=g)
    dx0 = torch.randn(N, H, W, C, generator=g)
    x = torch.zeros(N, H, W, C, dtype=torch.float64, requires_grad=True)
    L.upsample2x(x).backward(dy[..., c_off:c_off + C].double())
    dyd = dy.cuda()
    worst = 0.0
    for acc in (False, True):
        dx = dx0.cuda()
        ops.upsample2x_bwd(dyd, Cy, c_off, dx, accumulate=acc)
        worst = max(worst, _close(dx, x.grad + dx0.double() if acc else x.grad, ("upsample_bwd", c_off, acc)))
    return worst


@pytest.mark.parametrize("i", [0, 1, 2])
def test_upsample2x_fwd_into_a_slice_past_the_cap(i):
    d = dict(PC.GLUE["upsample_fwd"].d)
    c_off = d.pop("c_offs")[i]
    assert (0, 4, d["Cy"] - d["C"])[i] == c_off
    _upsample_fwd(c_off=c_off, **d)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_upsample2x_bwd_from_a_slice_past_the_cap(i):
    """assign and accumulate, against autograd of L.upsample2x"""
    d = dict(PC.GLUE["upsample_bwd"].d)
    c_off = d.pop("c_offs")[i]
    assert (0, 4, d["Cy"] - d["C"])[i] == c_off
    print("PAST_CAP_WORST upsample_bwd", c_off, _upsample_bwd(c_off=c_off, **d))


@pytest.mark.parametrize("N,H,W,C,Cy,c_off", [(1, 1, 1, 4, 4, 0), (1, 1, 1, 4, 12, 8), (2, 3, 5, 4, 8, 4), (1, 5, 3, 8, 20, 12)])
def test_upsample2x_small_edges(N, H, W, C, Cy, c_off):
    _upsample_fwd(N, H, W, C, Cy, c_off)
    _upsample_bwd(N, H, W, C, Cy, c_off)


# ---- space_to_depth(2) --------------------------------------------------------------------------------------------------
def _s2d(N, H, W, C, Cy, c_off, seed=5):
    from tf2_yolo_amd import ops
    g = _gen(seed)
    x = torch.randn(N, H, W, C, generator=g)
    y = torch.full((N, H // 2, W // 2, Cy), SENT, device="cuda")
    ops.space_to_depth2_fwd(x.cuda(), y, Cy, c_off)
    ref = torch.full((N, H // 2, W // 2, Cy), SENT)
    ref[..., c_off:c_off + 4 * C] = L.space_to_depth2(x)
    _same(y, ref, ("s2d_fwd", N, H, W, C, Cy, c_off))
    dy = torch.randn(N, H // 2, W // 2, Cy, generator=g)
    dx0 = torch.randn(N, H, W, C, generator=g)
    xg = torch.zeros(N, H, W, C, dtype=torch.float64, requires_grad=True)
    L.space_to_depth2(xg).backward(dy[..., c_off:c_off + 4 * C].double())
    grad = xg.grad.float()                                     # a permutation of fp32 values: exact
    dyd = dy.cuda()
    for acc in (False, True):
        dx = dx0.cuda()
        ops.space_to_depth2_bwd(dyd, Cy, c_off, dx, accumulate=acc)
        _same(dx, dx0 + grad if acc else grad, ("s2d_bwd", N, H, W, C, Cy, c_off, acc))


def test_space_to_depth2_slice_past_the_cap():
    _s2d(**PC.GLUE["s2d"].d)


@pytest.mark.parametrize("N,H,W,C,Cy,c_off", [(1, 2, 2, 1, 4, 0), (1, 2, 2, 1, 7, 3), (2, 4, 6, 2, 9, 1), (1, 6, 2, 5, 24, 4),
                                              (2, 2, 4, 4, 16, 0)])
def test_space_to_depth2_small_edges(N, H, W, C, Cy, c_off):
    _s2d(N, H, W, C, Cy, c_off)


# ---- max pooling ----------------------------------------------------------------------------------------------------------
def _first_winners(m, k, s, pt, pl, Ho, Wo):
    """flat offsets into m [N, H, W, C] of the FIRST maximum of every window in row-major window order (padding never
    wins), [N, Ho, Wo, C]: Tensor.unfold over the -inf-padded planes, argmax = the first maximal index"""
    N, H, W, C = m.shape
    pb, pr = max((Ho - 1) * s + k - H - pt, 0), max((Wo - 1) * s + k - W - pl, 0)
    mp = F.pad(m.float().permute(0, 3, 1, 2), (pl, pr, pt, pb), value=-math.inf)
    win = mp.unfold(2, k, s).unfold(3, k, s)[:, :, :Ho, :Wo]             # [N, C, Ho, Wo, k, k], a view
    idx = win.reshape(N, C, Ho, Wo, k * k).argmax(-1)
    h = torch.arange(Ho).view(1, 1, Ho, 1) * s + idx // k - pt
    w = torch.arange(Wo).view(1, 1, 1, Wo) * s + idx % k - pl
    assert int(h.min()) >= 0 and int(h.max()) < H and int(w.min()) >= 0 and int(w.max()) < W
    off = ((torch.arange(N).view(N, 1, 1, 1) * H + h) * W + w) * C + torch.arange(C).view(1, C, 1, 1)
    return off.permute(0, 2, 3, 1).contiguous()


def _general_pool(N, H, W, C, k, s, pad, Cy, c_off, seed=6):
    """yolo_maxpool_fwd on a shape its special kernels decline, written into a channel slice; values, winners, and the two
    backward forms against the scatter of dy to the oracle's winners"""
    from tf2_yolo_amd import ops
    g = _gen(seed + k + s)
    m = _ties(g, (N, H, W, C))
    ref = L.maxpool(m, k, s, pad)
    Ho, Wo = ref.shape[1], ref.shape[2]
    pt = L.same_pad(H, k, s)[1] if pad == "same" else 0
    pl = L.same_pad(W, k, s)[1] if pad == "same" else 0
    win = _first_winners(m, k, s, pt, pl, Ho, Wo)
    assert torch.equal(m.reshape(-1)[win.reshape(-1)].reshape(ref.shape), ref)      # (the reference agrees with itself)
    md = m.float().cuda()
    out = torch.full((N, Ho, Wo, Cy), SENT, device="cuda")
    arg = torch.full((N, Ho, Wo, C), -5, device="cuda", dtype=torch.int32)
    ops.maxpool_fwd(md, k, s, pt, pl, Ho, Wo, out, Cy, c_off, arg)
    want = torch.full((N, Ho, Wo, Cy), SENT)
    want[..., c_off:c_off + C] = ref.float()
    _same(out, want, ("maxpool_fwd", k, s, pad))
    _same(arg.long(), win, ("maxpool winners", k, s, pad))
    dy = torch.randn(N, Ho, Wo, Cy, generator=g)
    scat = torch.zeros(N * H * W * C, dtype=torch.float64)
    scat.index_add_(0, win.reshape(-1), dy[..., c_off:c_off + C].double().reshape(-1))
    dyd = dy.cuda()
    dx = torch.zeros(N, H, W, C, device="cuda")
    ops.maxpool_bwd(dyd, N, Ho, Wo, C, Cy, c_off, arg, dx)
    worst = _close(dx, scat, ("maxpool_bwd", k, s, pad))
    if s == 1 and pad == "same":
        dx = torch.ones(N, H, W, C, device="cuda")                                   # dx += ...
        ops.maxpool_bwd_same(dyd, N, H, W, C, Cy, c_off, arg, k, pt, pl, dx)
        worst = max(worst, _close(dx, scat + 1.0, ("maxpool_bwd_same", k, s, pad)))
    return worst


@pytest.mark.parametrize("name", ["pool_2x2s2_valid_odd", "pool_2x2s1_same", "pool_5x5s1_same"])
def test_general_maxpool_into_a_slice_past_the_cap(name):
    """2x2 s2 'valid' on an odd size, 2x2 s1 'same', and 5x5 s1 'same' on a map of more than 1024 pixels, which the plane
    kernel declines: maxpool_fwd_kernel / maxpool_bwd_kernel with three passes per thread"""
    print("PAST_CAP_WORST", name, _general_pool(**PC.GLUE[name].d))


@pytest.mark.parametrize("N,H,W,C,k,s,pad,Cy,c_off", [(1, 2, 2, 1, 2, 2, "valid", 3, 2), (2, 7, 5, 5, 2, 2, "valid", 9, 4),
                                                      (1, 5, 7, 2, 2, 1, "same", 4, 1), (1, 9, 9, 4, 5, 1, "same", 8, 4),
                                                      (2, 6, 4, 4, 2, 2, "same", 4, 0)])
def test_general_maxpool_small_edges(N, H, W, C, k, s, pad, Cy, c_off):
    _general_pool(N, H, W, C, k, s, pad, Cy, c_off)


def _pool2x2_fast_vs_general(N, H, W, C, seed=7):
    from tf2_yolo_amd import ops
    g = _gen(seed)
    m = _ties(g, (N, H, W, C))
    Ho, Wo = H // 2, W // 2
    md = m.float().cuda()
    out = torch.empty(N, Ho, Wo, C, device="cuda")
    arg = torch.full((N, Ho, Wo, C), -5, device="cuda", dtype=torch.int32)
    ops.maxpool_fwd(md, 2, 2, 0, 0, Ho, Wo, out, C, 0, arg)                  # Cy == C, c_off == 0: the fast path
    wide = torch.full((N, Ho, Wo, C + 4), SENT, device="cuda")
    arg2 = torch.full((N, Ho, Wo, C), -5, device="cuda", dtype=torch.int32)
    ops.maxpool_fwd(md, 2, 2, 0, 0, Ho, Wo, wide, C + 4, 4, arg2)            # Cy = C + 4: falls through to the general kernel
    assert torch.equal(wide[..., 4:], out) and torch.equal(arg, arg2) and bool((wide[..., :4] == SENT).all())
    _same(out, L.maxpool(m, 2, 2, "valid").float(), "2x2 values")
    _same(arg.long(), _first_winners(m, 2, 2, 0, 0, Ho, Wo), "2x2 winners")
    dyd = torch.randn(N, Ho, Wo, C, generator=g).cuda()
    scat = torch.zeros(N, H, W, C, device="cuda")
    ops.maxpool_bwd(dyd, N, Ho, Wo, C, C, 0, arg, scat)
    dm = torch.full((N, H, W, C), SENT, device="cuda")
    ops.maxpool2x2_bwd(dyd, N, Ho, Wo, C, arg, dm, False)                    # assign: overwrites every element
    assert torch.equal(dm, scat)
    base = torch.randn(N, H, W, C, generator=g).cuda()
    acc = base.clone()
    ops.maxpool2x2_bwd(dyd, N, Ho, Wo, C, arg, acc, True)
    assert torch.equal(acc, base + scat)


def test_maxpool2x2_fast_path_equals_the_general_kernel_past_the_cap():
    _pool2x2_fast_vs_general(**PC.GLUE["pool2x2_fast"].d)


@pytest.mark.parametrize("N,H,W,C", [(1, 2, 2, 4), (2, 6, 10, 4), (1, 4, 2, 8)])
def test_maxpool2x2_fast_path_small_edges(N, H, W, C):
    _pool2x2_fast_vs_general(N, H, W, C)


@pytest.mark.parametrize("name", ["bn_act_pool", "bn_act_pool_planes"])
def test_bn_act_maxpool2x2_past_the_cap(name):
    """BatchNorm apply + LeakyReLU + MaxPooling2D(2, 2) in one launch against BN, then activation, then L.maxpool in float64;
    the recorded winner lies in its window and holds the pooled value; the planes decode to the pooled tensor"""
    from planes_util import planes_to_dense
    from tf2_yolo_amd import ops
    d = PC.GLUE[name].d
    N, H, W, C = d["N"], d["H"], d["W"], d["C"]
    Ho, Wo = H // 2, W // 2
    P = N * Ho * Wo
    g = _gen(8)
    y = torch.randn(N, H, W, C, generator=g) * 2 + 0.3
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g)
    a = torch.cat([L.leaky(y[b:b + 1].double() * scale.double() + shift.double()) for b in range(N)])
    ref = L.maxpool(a, 2, 2, "valid")
    bound = float(a.abs().max()) * 1.01
    bnb = torch.tensor([bound], device="cuda").view(torch.int32)
    out = torch.full((N, Ho, Wo, C), SENT, device="cuda")
    arg = torch.full((N, Ho, Wo, C), -5, device="cuda", dtype=torch.int32)
    pl = torch.full((ops.planes_bytes(P, C),), 0x55, device="cuda", dtype=torch.uint8) if name.endswith("planes") else None
    ob = torch.zeros(1, device="cuda")
    ops.bn_act_maxpool2x2_fwd(y.cuda(), C, scale.cuda(), shift.cuda(), 1, arg, out=out, planes=pl, bn_bound=bnb, out_bound=ob)
    print("PAST_CAP_WORST", name, _close(out, ref, name))
    al = arg.cpu().long()
    assert int(al.min()) >= 0 and int(al.max()) < y.numel()
    pix, ch = al // C, al % C
    assert torch.equal(ch, torch.arange(C).expand_as(ch))
    wi, hi, bi = pix % W, (pix // W) % H, pix // (W * H)
    assert torch.equal(hi // 2, torch.arange(Ho).view(1, Ho, 1, 1).expand_as(hi))
    assert torch.equal(wi // 2, torch.arange(Wo).view(1, 1, Wo, 1).expand_as(wi))
    assert torch.equal(bi, torch.arange(N).view(N, 1, 1, 1).expand_as(bi))
    _close(a.reshape(-1)[al.reshape(-1)], ref, "the winner holds the pooled value")
    if pl is not None:
        dense, b, s, tail0 = planes_to_dense(pl.cpu(), P, C)
        assert tail0 and b == float(bnb.view(torch.float32)) == float(ob) and b >= float(ref.abs().max())
        r = out.double().cpu().reshape(-1, C)
        assert ((dense - r).abs() <= torch.maximum(2.0 ** -22 * r.abs(), torch.tensor(2.0 ** -25 / s, dtype=torch.float64))).all()


# ---- stand-alone activations, axpy, fill, optimizer steps --------------------------------------------------------------------
def _act_ref(z, act):
    return z if act == 0 else L.leaky(z) if act == 1 else L.mish(z)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n", [PC.GLUE["act"].d["n"], 1, 5, 257])
def test_act_fwd_bwd(n, act):
    """ops.act_fwd / ops.act_bwd (conv units without BatchNorm): linear, LeakyReLU, Mish against L.leaky / L.mish and autograd"""
    from tf2_yolo_amd import ops
    g = _gen(9 + act)
    z = (torch.randn(n, generator=g) * 3).double().requires_grad_(True)
    dout = torch.randn(n, generator=g)
    out = _act_ref(z, act)
    out.backward(dout.double())
    zd = z.detach().float().cuda()
    w1 = _close(ops.act_fwd(zd, act), out, ("act_fwd", act))
    w2 = _close(ops.act_bwd(zd, dout.cuda(), act), z.grad, ("act_bwd", act))
    if act == 0:
        _same(ops.act_fwd(zd, act), z.detach().float())
        _same(ops.act_bwd(zd, dout.cuda(), act), dout)
    print("PAST_CAP_WORST act", n, act, w1, w2)


def test_mish_accuracy_on_a_fixed_grid():
    """act.hpp's Mish (exp2 of the scaled argument, one rational function of e = exp(-|z|)) and its derivative against float64
    z tanh(softplus(z)) and the analytic derivative: a step of 1/64 over [-30, 30] and both signs of the points where exp2
    approaches underflow. The worst error and its z are printed (DESIGN.md records them)."""
    from tf2_yolo_amd import ops
    pts = torch.tensor([1e-6, 1e-3, 1.19, 20.0, 60.0, 87.0, 88.5], dtype=torch.float64)
    z = torch.cat([torch.arange(-30 * 64, 30 * 64 + 1, dtype=torch.float64) / 64, pts, -pts]).float()
    zz = z.double()
    t = torch.tanh(L.softplus(zz))
    ref = zz * t
    dref = t + zz * (1 - t * t) * torch.sigmoid(zz)
    zd = z.cuda()
    got = ops.act_fwd(zd, 2).double().cpu()
    dgot = ops.act_bwd(zd, torch.ones_like(zd), 2).double().cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dgot).all())
    for what, a, b in (("mish", got, ref), ("mish'", dgot, dref)):
        err = (a - b).abs() / b.abs().clamp(min=1.0)
        i = int(err.argmax())
        print(f"MISH_ACCURACY {what}: worst error {err[i].item():.3e} (relative to max(1, |ref|)) at z = {float(z[i])!r}")
        assert err[i].item() <= TOL, (what, err[i].item(), float(z[i]))


@pytest.mark.parametrize("n", [PC.GLUE["axpy_r0"].d["n"], PC.GLUE["axpy_r1"].d["n"], PC.GLUE["axpy_r3"].d["n"], 1, 3, 4, 7])
def test_axpy_and_fill(n):
    """a += b bit-equal to fp32 a + b for n % 4 in {0, 1, 3}; fill sets its n elements; what lies beyond n stays"""
    from tf2_yolo_amd import ops
    g = _gen(10)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    buf = torch.full((n + 8,), SENT, device="cuda")
    buf[:n] = a.cuda()
    ops.axpy(buf[:n], b.cuda())
    _same(buf[:n], a + b, "axpy")
    assert bool((buf[n:] == SENT).all())
    ops.fill(buf[:n], 3.25)
    assert bool((buf[:n] == 3.25).all()) and bool((buf[n:] == SENT).all())


def test_fill_past_the_cap():
    from tf2_yolo_amd import ops
    n = PC.GLUE["fill"].d["n"]
    buf = torch.full((n + 8,), SENT, device="cuda")
    ops.fill(buf[:n], -0.75)
    assert bool((buf[:n] == -0.75).all()) and bool((buf[n:] == SENT).all())


@pytest.mark.parametrize("n", [PC.GLUE["sgd"].d["n"], 7])
def test_sgd_step_with_a_ragged_tail(n):
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(11)
    p, gr = rng.standard_normal(n), rng.standard_normal(n)
    pd = torch.tensor(p, dtype=torch.float32, device="cuda")
    gd = torch.tensor(gr, dtype=torch.float32, device="cuda")
    g0 = gd.clone()
    ops.sgd_step(pd, gd, 0.1, grad_scale=0.5, zero_grad=False)
    assert torch.equal(gd, g0)
    assert np.abs(pd.cpu().numpy() - (p - 0.1 * 0.5 * gr)).max() < 1e-5
    ops.sgd_step(pd, gd, 0.1, grad_scale=0.5, zero_grad=True)
    assert float(gd.abs().max()) == 0.0
    assert np.abs(pd.cpu().numpy() - (p - 2 * 0.1 * 0.5 * gr)).max() < 1e-5


@pytest.mark.parametrize("dev_hyper", [False, True])
@pytest.mark.parametrize("n", [PC.GLUE["adam"].d["n"], 7, 1])
def test_adam_step_with_a_ragged_tail(n, dev_hyper):
    """adam_step / adam_step_dev with n % 4 != 0 against the Keras formula of test_adam_matches_keras_formula; zero_grad True
    zeroes g, False leaves it as it was"""
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(12)
    p = rng.standard_normal(n)
    pd = torch.tensor(p, dtype=torch.float32, device="cuda")
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pm, mm, vv = p.copy(), np.zeros(n), np.zeros(n)
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-7, 0.5
    for step, zero in ((1, False), (2, True)):
        gr = rng.standard_normal(n)
        gd = torch.tensor(gr, dtype=torch.float32, device="cuda")
        g0 = gd.clone()
        if dev_hyper:
            hyper = torch.tensor([ops.adam_lr_t(lr, step, b1, b2), b1, b2, eps, gs], dtype=torch.float32, device="cuda")
            ops.adam_step_dev(pd, gd, m, v, hyper, zero_grad=zero)
        else:
            ops.adam_step(pd, gd, m, v, lr, step, beta1=b1, beta2=b2, eps=eps, grad_scale=gs, zero_grad=zero)
        assert float(gd.abs().max()) == 0.0 if zero else torch.equal(gd, g0)
        gg = gr * gs
        mm = b1 * mm + (1 - b1) * gg
        vv = b2 * vv + (1 - b2) * gg * gg
        pm -= lr * np.sqrt(1 - b2 ** step) / (1 - b1 ** step) * mm / (np.sqrt(vv) + eps)
    assert np.abs(pd.cpu().numpy() - pm).max() < 1e-5
    assert np.abs(m.cpu().numpy() - mm).max() < 1e-5 and np.abs(v.cpu().numpy() - vv).max() < 1e-5


# ---- detection-head activations ------------------------------------------------------------------------------------------
def _head(version, P, A, C, danchors=False, seed=13):
    from tf2_yolo_amd import ops
    g = _gen(seed + version)
    D = 5 * A + C if version == 1 else A * (5 + C)
    t = torch.randn(P, D, generator=g, dtype=torch.float64).requires_grad_(True)
    anchors = torch.rand(A, 2, generator=g, dtype=torch.float64) + 0.1
    if version == 1:
        y = torch.cat([torch.sigmoid(t[:, :5 * A]), torch.softmax(t[:, 5 * A:], dim=-1)], dim=-1)
    else:
        tt = t.reshape(P, A, 5 + C)
        cls = torch.softmax(tt[..., 5:], dim=-1) if version == 2 else torch.sigmoid(tt[..., 5:])
        y = torch.cat([torch.sigmoid(tt[..., 0:2]), torch.exp(tt[..., 2:4]) * anchors, torch.sigmoid(tt[..., 4:5]),
                       cls], dim=-1).reshape(P, D)
    dy = torch.randn(P, D, generator=g, dtype=torch.float64)
    y.backward(dy)
    anc = anchors.float().reshape(-1).cuda() if version != 1 else None
    td, dyd = t.detach().float().cuda(), dy.float().cuda()
    yd = ops.head_act_fwd(td, A, C, version, anc)
    worst = _close(yd, y, ("head_act_fwd", version))
    worst = max(worst, _close(ops.head_act_bwd(yd, dyd, A, C, version, anc), t.grad, ("head_act_bwd", version)))
    if danchors:
        da = torch.zeros(2 * A, device="cuda")
        ops.head_act_bwd(yd, dyd, A, C, version, anc, danchors=da)
        tt = t.detach().reshape(P, A, 5 + C)
        ref = (dy.reshape(P, A, 5 + C)[..., 2:4] * torch.exp(tt[..., 2:4])).sum(0).reshape(-1)
        worst = max(worst, _close(da, ref, "danchors"))
    return worst


@pytest.mark.parametrize("name", ["head_v1", "head_v2", "head_v2_softmax", "head_v3", "head_v4", "head_v4_danchors"])
def test_head_act_past_the_cap(name):
    """logits from a normal distribution, anchors in [0.1, 1.1]; head_v4_danchors: more than 2 x 65 536 pixels, past the
    256-workgroup cap of head_danchor_kernel"""
    d = PC.GLUE[name].d
    print("PAST_CAP_WORST", name, _head(d["version"], d["P"], d["A"], d["C"], danchors=name.endswith("danchors")))


@pytest.mark.parametrize("version,A,C", [(1, 1, 1), (1, 2, 5), (2, 1, 1), (2, 5, 2), (3, 1, 1), (3, 3, 5), (4, 1, 1), (4, 3, 2)])
def test_head_act_one_pixel(version, A, C):
    _head(version, 1, A, C, danchors=version == 4)


# ---- BatchNorm with C % 8 == 4 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("C,P", [(4, 105), (12, 105), (20, 105), (12, PC.GLUE["bn_c12"].d["P"]), (20, PC.GLUE["bn_c20"].d["P"])])
def test_bn_act_fwd_bwd_with_c_mod_8_equal_4(C, P, act, use_res):
    """bn_act_fwd_kernel / bn_bwd_apply_kernel (the float4 forms taken when C % 8 == 4) with the oracle of
    test_bn_act_train_fwd_bwd, at 105 pixels and with P C / 4 past the cap"""
    from tf2_yolo_amd import ops
    assert C % 8 == 4
    g = _gen(C + act + P % 7)
    shape = (3, 7, 5, C) if P == 105 else (1, 1, P, C)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(shape, generator=g, dtype=torch.float64) if use_res else None
    z, mean, var = L.batchnorm_train(x, gamma, beta)
    a = L.leaky(z) if act == 1 else L.mish(z)
    out = a + res if use_res else a
    dout = torch.randn(shape, generator=g, dtype=torch.float64)
    out.backward(dout)

    dev = "cuda"
    xd = x.detach().float().to(dev)
    stats = torch.zeros(64 * 2 * C, device=dev, dtype=torch.float64)
    red = torch.zeros(513 * 2 * C, device=dev, dtype=torch.float64)
    f = lambda: torch.empty(C, device=dev)
    scale, shift, smean, sinv = f(), f(), f(), f()
    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    gd, bd = gamma.detach().float().to(dev), beta.detach().float().to(dev)
    ops.bn_stats(xd, C, stats)
    ops.bn_finalize(stats, P, C, gd, bd, mm, mv, scale, shift, smean, sinv)
    o = ops.bn_act_fwd(xd, C, scale, shift, act, None if res is None else res.float().to(dev))
    w = {"out": _close(o, out, "out"), "mean": _close(smean, mean, "mean"), "moving_mean": _close(mm, 0.01 * mean, "moving mean"),
         "moving_var": _close(mv, 0.99 + 0.01 * var, "moving variance")}
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dx = ops.bn_act_bwd(xd, dout.float().to(dev), C, gd, scale, shift, smean, sinv, act, red, dg, db)
    w.update(dx=_close(dx, x.grad, "dx"), dgamma=_close(dg, gamma.grad, "dgamma"), dbeta=_close(db, beta.grad, "dbeta"))
    print("PAST_CAP_WORST bn", C, P, act, use_res, {k: float(f"{v:.2e}") for k, v in w.items()})


# ---- labels, IoU -----------------------------------------------------------------------------------------------------------------
def test_down2xlabel_past_the_cap():
    from oracle import tools as T
    from tf2_yolo_amd import ops
    d = PC.GLUE["down2xlabel"].d
    rng = np.random.default_rng(14)
    lab = rng.random((d["N"], d["gh"], d["gw"], d["ch"]))
    lab[..., 4] = rng.random(lab.shape[:3]) < 0.3
    lab[lab[..., 4] == 0] = 0
    o64, o32 = ops.down2xlabel(torch.from_numpy(lab).cuda())
    ref = T.down2xlabel(lab)
    assert np.array_equal(o64.cpu().numpy(), ref) and np.array_equal(o32.cpu().numpy(), ref.astype(np.float32))


def test_cal_iou_past_the_cap():
    """the broadcasting IoU / DIoU kernel on 1031 x 1061 pairs against oracle.tools.cal_iou, bit for bit (float64, and
    float32 operands as NumPy computes them)"""
    from oracle import tools as OT
    from tf2_yolo_amd import ops
    d = PC.GLUE["cal_iou"].d
    rng = np.random.default_rng(15)

    def boxes(n):
        return np.concatenate([rng.random((n, 2)), rng.random((n, 2)) * 0.5 + 0.02], axis=1)
    a, b = boxes(d["M"]).reshape(-1, 1, 4), boxes(d["K"]).reshape(1, -1, 4)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for mode in (1, 2):
        got = ops.cal_iou(ad, bd, mode=mode).cpu().numpy()
        assert got.shape == (d["M"], d["K"]) and np.array_equal(got, OT.cal_iou(a, b, mode))
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    got = ops.cal_iou(torch.from_numpy(a32).cuda(), torch.from_numpy(b32).cuda(), mode=2).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, OT.cal_iou(a32, b32, 2))


# ---- rejections on the host: YOLO_REQUIRE returns before any launch ----------------------------------------------------
def test_launchers_reject_bad_slices_before_launching():
    from tf2_yolo_amd import ops
    from tf2_yolo_amd._lib import YoloHipError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(YoloHipError):
        ops.upsample2x_fwd(z(1, 2, 2, 6), z(1, 4, 4, 8), 8, 0)                 # C % 4 != 0
    with pytest.raises(YoloHipError):
        ops.upsample2x_fwd(z(1, 2, 2, 4), z(1, 4, 4, 12), 12, 2)               # c_off % 4 != 0
    with pytest.raises(YoloHipError):
        ops.upsample2x_bwd(z(1, 4, 4, 8), 8, 0, z(1, 2, 2, 6))
    with pytest.raises(YoloHipError):
        ops.upsample2x_bwd(z(1, 4, 4, 12), 12, 2, z(1, 2, 2, 4))
    with pytest.raises(YoloHipError):
        ops.space_to_depth2_fwd(z(1, 3, 4, 2), z(1, 1, 2, 8), 8, 0)            # odd H
    with pytest.raises(YoloHipError):
        ops.space_to_depth2_bwd(z(1, 1, 2, 8), 8, 0, z(1, 3, 4, 2))
    with pytest.raises(YoloHipError):
        ops.copy_channels_in(z(5, 8), 8, z(5, 12), 12, 8)                      # c_off + C beyond the wide tensor
    with pytest.raises(YoloHipError):
        ops.copy_channels_out(z(5, 12), 12, 8, z(5, 8), 8)
    with pytest.raises(YoloHipError):
        ops.maxpool2x2_bwd(z(1, 1, 1, 6), 1, 1, 1, 6, torch.zeros(1, 1, 1, 6, device="cuda", dtype=torch.int32), z(1, 2, 2, 6),
                           False)                                              # C % 4 != 0
