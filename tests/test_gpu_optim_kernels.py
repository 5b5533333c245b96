"""Kernel level: the deterministic gradient norms, the clip factors, and the Adam / SGD update kernels that read their
scalars from device memory (csrc/optim.hip), against the float64 restatement of the Keras rules in optimizer_ref.py.

Layout of every case: variables of 1, 3, 64, 65, 4099 and 70 000 floats at 64-float aligned offsets (a scalar tail, exactly
and just over one alignment unit, several float4 passes with a tail, several chunks with a partial last one). The padding of
the gradient is poisoned with 1e3 -- one padding element inside a norm would be seen at once -- and the padding of every
buffer the update writes holds a sentinel that must survive."""
import math

import numpy as np
import pytest
import torch

import optimizer_ref as R

pytestmark = pytest.mark.gpu

VARS, TOTAL = R.layout()
MASK = R.mask(VARS, TOTAL)
B1, B2, EPS = 0.9, 0.999, 1e-7
SENTINEL = {"p": 7.0, "m": -3.0, "v": 5.0, "vhat": 9.0, "a": 11.0}
GS = 0.5                      # grad_scale = 1/world of two ranks
# per-step gradient scales: the norms of steps 1 and 3 exceed the thresholds below, those of step 2 do not
STEP_SCALE = (1.0, 0.02, 1.0)
# thresholds that bite on some variables / steps / elements and not on others (norm of GS * N(0,1) over n elements
# ~ 0.5 sqrt(n): 0.5 .. 4 for the four small variables, 32 and 132 for the large ones, 136 globally)
CLIPS = {"none": {}, "clipnorm": {"clipnorm": 5.0}, "global_clipnorm": {"global_clipnorm": 50.0},
         "clipvalue": {"clipvalue": 0.6}}


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def data():
    """float32 host data shared by every case, never modified: start parameters and three gradients with poisoned padding"""
    rng = np.random.default_rng(0)
    p = rng.standard_normal(TOTAL).astype(np.float32)
    gs = []
    for s in STEP_SCALE:
        g = (rng.standard_normal(TOTAL) * s).astype(np.float32)
        g[~MASK] = 1e3
        gs.append(g)
    return {"p": p, "g": gs}


def _padded(values, name):
    a = np.array(values, dtype=np.float32)
    a[~MASK] = SENTINEL[name]
    return _dev(a)


def _hyper(lr, gs=GS, mu=0.0, thr=0.0):
    return _dev([lr, B1, B2, EPS, gs, mu, thr, 0.0])


def _mode(clip):
    from tf2_yolo_amd import ops
    name = next(iter(clip), None)
    return ({None: ops.CLIP_NONE, "clipnorm": ops.CLIP_NORM, "global_clipnorm": ops.CLIP_GLOBAL,
             "clipvalue": ops.CLIP_VALUE}[name], clip.get(name, 0.0))


def _norm_and_factors(ops, g, table, hyper, mode):
    """norm -> factors, as the optimizers enqueue them; returns (factors, norm_out) or (None, None)"""
    if mode not in (ops.CLIP_NORM, ops.CLIP_GLOBAL):
        return None, None
    factors = torch.full((table.n_vars if mode == ops.CLIP_NORM else 1,), float("nan"), device="cuda")
    norm = torch.full((1,), float("nan"), device="cuda")
    ops.grad_sqnorm(g, table)
    ops.clip_factors(table, hyper, mode, factors, norm_out=norm)
    return factors, norm


# ---- squared norms ----
@pytest.mark.parametrize("chunk,extra", [(8192, 0), (64, 0), (8192, 40)])
def test_squared_norms_match_float64_and_are_reproducible(chunk, extra):
    """per-variable and global squared norms against the EXACT sum (math.fsum of the exact float64 products) of the same
    float32 data, to 1e-12 relative: products of two floats are exact in double, and a variable's sum passes through at
    most ~32 (thread) + 8 (wave tree, wave sums) + chunks-of-the-variable additions, each within 2^-53.
    Cases: the default 8192-float chunks (one to nine chunks per variable); 64-float chunks (1094 partials for the largest
    variable: stage 2 walks them 64 at a time); 40 more small variables (stage 2 gives each wave several variables).
    Bit-identical across two calls. The launch geometry is no parameter of the call: one workgroup per chunk of the table,
    and the chunk size is part of the table -- of WHAT is summed in which order -- so it is not varied under bit equality."""
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(1)
    sizes = R.SIZES + tuple(int(s) for s in rng.integers(1, 300, size=extra))
    variables, total = R.layout(sizes)
    g = rng.standard_normal(total).astype(np.float32)
    g[~R.mask(variables, total)] = 1e3
    table = ops.ChunkTable(variables, chunk=chunk)
    gd = _dev(g)
    got = []
    for _ in range(2):
        table.var_sq.fill_(float("nan")); table.total_sq.fill_(float("nan")); table.workspace.fill_(float("nan"))
        ops.grad_sqnorm(gd, table)
        got.append((table.var_sq.cpu().numpy().copy(), float(table.total_sq.cpu()[0])))
    want = np.array([math.fsum(float(x) * float(x) for x in g[o:o + s]) for o, s in variables])
    rel = np.abs(got[0][0] - want) / want
    rel_tot = abs(got[0][1] - math.fsum(want)) / math.fsum(want)
    print(f"\n[sqnorm chunk {chunk}, {len(variables)} variables] max rel err per variable {rel.max():.3e}, global {rel_tot:.3e}")
    assert rel.max() <= 1e-12 and rel_tot <= 1e-12
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    assert torch.equal(gd, _dev(g))                      # the norm only reads


# ---- every optimizer form x every clip mode, three steps ----
OPTS = {"adam": dict(kind="adam", amsgrad=False), "adam_amsgrad": dict(kind="adam", amsgrad=True),
        "sgd": dict(kind="sgd", mu=0.0, nesterov=False), "sgd_momentum": dict(kind="sgd", mu=0.9, nesterov=False),
        "sgd_nesterov": dict(kind="sgd", mu=0.9, nesterov=True)}


@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("opt", list(OPTS))
def test_update_matches_keras_rule(opt, clip, data):
    """three steps; parameters within 1e-5 absolute of the float64 rule (the bar and the data scale of
    test_gpu_elementwise.py::test_adam_matches_keras_formula), gradients zeroed on variable elements, sentinels in the
    padding of every written buffer intact, the factors exactly 1 where the norm is at or below the threshold, and the
    threshold biting somewhere and not somewhere else"""
    from tf2_yolo_amd import ops
    o, ckw = OPTS[opt], CLIPS[clip]
    mode, thr = _mode(ckw)
    table = ops.ChunkTable(VARS)
    lr = 1e-3 if o["kind"] == "adam" else 1e-2
    p = _padded(data["p"], "p")
    if o["kind"] == "adam":
        ref = R.AdamRef(data["p"], VARS, lr=lr, b1=B1, b2=B2, eps=EPS, amsgrad=o["amsgrad"], **ckw)
        m, v = _padded(np.zeros(TOTAL), "m"), _padded(np.zeros(TOTAL), "v")
        vhat = _padded(np.zeros(TOTAL), "vhat") if o["amsgrad"] else None
        written = {"p": p, "m": m, "v": v, "vhat": vhat}
    else:
        ref = R.SGDRef(data["p"], VARS, lr=lr, momentum=o["mu"], nesterov=o["nesterov"], **ckw)
        a = _padded(np.zeros(TOTAL), "a") if o["mu"] > 0 else None
        written = {"p": p, "a": a}
    bit, free = 0, 0
    for step, g_h in enumerate(data["g"], start=1):
        g = _dev(g_h)
        hyper = _hyper(ops.adam_lr_t(lr, step, B1, B2) if o["kind"] == "adam" else lr, mu=o.get("mu", 0.0), thr=thr)
        factors, norm = _norm_and_factors(ops, g, table, hyper, mode)
        if o["kind"] == "adam":
            ops.adam_step_clip(p, g, m, v, table, hyper, factors=factors, clip_mode=mode, vhat=vhat)
        else:
            ops.sgd_step_clip(p, g, table, hyper, accum=a, nesterov=o["nesterov"], factors=factors, clip_mode=mode)
        gnorm = ref.step(g_h, grad_scale=GS)
        g_after = g.cpu().numpy()
        assert (g_after[MASK] == 0.0).all() and (g_after[~MASK] == 1e3).all()      # zeroed on variables, padding untouched
        if factors is not None:
            assert float(norm[0]) == pytest.approx(gnorm, rel=1e-6)
            per, _ = R.sq_norms(g_h.astype(np.float64) * GS, VARS)
            norms = np.sqrt(per) if mode == ops.CLIP_NORM else np.array([gnorm])
            f = factors.cpu().numpy()
            np.testing.assert_allclose(f, thr / np.maximum(norms, thr), rtol=2e-7)
            assert (f[norms <= thr] == 1.0).all()
            bit += int((norms > thr).sum())
            free += int((norms <= thr).sum())
        elif mode == ops.CLIP_VALUE:
            x = np.abs(g_h[MASK].astype(np.float64) * GS)
            bit += int((x > thr).sum())
            free += int((x <= thr).sum())
    if mode != ops.CLIP_NONE:
        assert bit > 0 and free > 0, (bit, free)
    err = np.abs(p.cpu().numpy().astype(np.float64) - ref.p)[MASK].max()
    print(f"\n[{opt} / {clip}] max |p - reference| after 3 steps {err:.3e}; clipped {bit}, not clipped {free}")
    assert err < 1e-5
    for name, t in written.items():
        if t is not None:
            h = t.cpu().numpy()
            assert (h[~MASK] == SENTINEL[name]).all(), f"padding of {name} was written"
            assert np.isfinite(h[MASK]).all()
    if o["kind"] == "adam":
        assert np.abs(m.cpu().numpy() - ref.m)[MASK].max() < 1e-6
        if o["amsgrad"]:
            assert np.abs(vhat.cpu().numpy() - ref.vhat)[MASK].max() < 1e-6
    elif a is not None:
        assert np.abs(a.cpu().numpy() - ref.a)[MASK].max() < 1e-6


# ---- a threshold that is never reached changes no bit ----
@pytest.mark.parametrize("mode_name", ["global_clipnorm", "clipnorm", "clipvalue"])
def test_threshold_never_reached_is_bit_identical_to_the_plain_kernels(mode_name, data):
    """threshold 1e30: p, m, v equal ops.adam_step_dev bit for bit over three steps, and for SGD without momentum p equals
    ops.sgd_step (on variable elements: the plain kernels also run over the padding). grad_scale is 0.5 here as everywhere
    in this file; a power of two, for which sgd_step's (lr * gs) * g and the new kernels' lr * (g * gs) round alike."""
    from tf2_yolo_amd import ops
    mode, thr = _mode({mode_name: 1e30})
    table = ops.ChunkTable(VARS)
    lr = 1e-3
    new = {k: _padded(data["p"] if k == "p" else np.zeros(TOTAL), k) for k in ("p", "m", "v")}
    old = {k: t.clone() for k, t in new.items()}
    sgd_new, sgd_old = new["p"].clone(), new["p"].clone()
    for step, g_h in enumerate(data["g"], start=1):
        hyper = _hyper(ops.adam_lr_t(lr, step, B1, B2), thr=thr)
        g = _dev(g_h)
        factors, _ = _norm_and_factors(ops, g, table, hyper, mode)
        if factors is not None:
            assert (factors == 1.0).all()
        ops.adam_step_clip(new["p"], g, new["m"], new["v"], table, hyper, factors=factors, clip_mode=mode)
        ops.adam_step_dev(old["p"], _dev(g_h), old["m"], old["v"], hyper[:5].clone())
        hyper_sgd = _hyper(1e-2, thr=thr)
        ops.sgd_step_clip(sgd_new, _dev(g_h), table, hyper_sgd, factors=factors, clip_mode=mode)
        ops.sgd_step(sgd_old, _dev(g_h), 1e-2, grad_scale=GS)
    k = torch.from_numpy(MASK).cuda()
    for name in ("p", "m", "v"):
        assert torch.equal(new[name][k], old[name][k]), name
    assert torch.equal(sgd_new[k], sgd_old[k])
    assert not torch.equal(new["p"][k], _dev(data["p"])[k])


@pytest.mark.parametrize("mode_name", ["global_clipnorm", "clipnorm"])
def test_zero_gradient_gives_factors_of_one_and_no_nan(mode_name):
    from tf2_yolo_amd import ops
    mode, thr = _mode({mode_name: 1.0})
    table = ops.ChunkTable(VARS)
    g = torch.zeros(TOTAL, device="cuda")
    hyper = _hyper(ops.adam_lr_t(1e-3, 1, B1, B2), thr=thr)
    factors, norm = _norm_and_factors(ops, g, table, hyper, mode)
    assert (factors == 1.0).all() and float(norm[0]) == 0.0
    assert (table.var_sq == 0.0).all() and float(table.total_sq[0]) == 0.0
    p0 = torch.randn(TOTAL, device="cuda")
    for amsgrad in (False, True):
        p, m, v = p0.clone(), torch.zeros(TOTAL, device="cuda"), torch.zeros(TOTAL, device="cuda")
        vhat = torch.zeros(TOTAL, device="cuda") if amsgrad else None
        ops.adam_step_clip(p, g, m, v, table, hyper, factors=factors, clip_mode=mode, vhat=vhat)
        assert torch.equal(p, p0) and not torch.isnan(m).any() and not torch.isnan(v).any()
    p, a = p0.clone(), torch.zeros(TOTAL, device="cuda")
    ops.sgd_step_clip(p, g, table, _hyper(1e-2, mu=0.9, thr=thr), accum=a, nesterov=True, factors=factors, clip_mode=mode)
    assert torch.equal(p, p0) and (a == 0.0).all()


def test_anchor_boxes_as_variables_and_the_ordered_global_sum():
    """the second table of a step: nine anchor boxes of 2 floats at offsets 2k (no 16-byte alignment: the scalar path), and
    the global norm that adds its sum to the parameters' -- parameters first"""
    from tf2_yolo_amd import ops
    rng = np.random.default_rng(2)
    g_h = rng.standard_normal(TOTAL).astype(np.float32)
    ag_h = rng.standard_normal(18).astype(np.float32)
    table, anch = ops.ChunkTable(VARS), ops.ChunkTable([(2 * i, 2) for i in range(9)])
    g, ag = _dev(g_h), _dev(ag_h)
    ops.grad_sqnorm(g, table)
    ops.grad_sqnorm(ag, anch)
    want = ag_h.astype(np.float64).reshape(9, 2) ** 2
    assert np.array_equal(anch.var_sq.cpu().numpy(), want[:, 0] + want[:, 1])
    hyper = _hyper(1e-2, gs=1.0, thr=1.0)
    f, fa, norm = torch.zeros(1, device="cuda"), torch.zeros(9, device="cuda"), torch.zeros(1, device="cuda")
    ops.clip_factors(table, hyper, ops.CLIP_GLOBAL, f, norm_out=norm, extra=anch)
    total = float(table.total_sq[0]) + float(anch.total_sq[0])
    assert total == pytest.approx(R.sq_norms(g_h, VARS)[1] + want.sum(), rel=1e-12)
    assert float(norm[0]) == pytest.approx(math.sqrt(total), rel=2e-7)          # (one rounding to float)
    assert float(f[0]) == pytest.approx(1.0 / math.sqrt(total), rel=2e-7)
    ops.clip_factors(anch, hyper, ops.CLIP_NORM, fa)
    np.testing.assert_allclose(fa.cpu().numpy(), 1.0 / np.maximum(np.sqrt(want.sum(1)), 1.0), rtol=2e-7)
    p = torch.zeros(18, device="cuda")
    ops.sgd_step_clip(p, ag, anch, hyper, factors=fa, clip_mode=ops.CLIP_NORM)
    ref = R.SGDRef(np.zeros(18), [(2 * i, 2) for i in range(9)], lr=1e-2, clipnorm=1.0)
    ref.step(ag_h)
    assert np.abs(p.cpu().numpy() - ref.p).max() < 1e-7 and (ag == 0.0).all()
