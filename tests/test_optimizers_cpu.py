"""Host side of the optimizers (no GPU): the learning-rate schedules and the legacy decay against their closed forms
(optimizer_ref.py), argument validation of Adam and SGD, and the chunk / variable table the norm and update kernels walk."""
import math

import numpy as np
import pytest

import optimizer_ref as R


# ---- schedules: steps 0, 1, a boundary, boundary + 1, past the end ----
@pytest.mark.parametrize("staircase", [False, True])
def test_exponential_decay(staircase):
    from tf2_yolo_amd.optimizers.schedules import ExponentialDecay
    s = ExponentialDecay(1e-2, decay_steps=10, decay_rate=0.5, staircase=staircase)
    for step in (0, 1, 10, 11, 1000):
        assert s(step) == pytest.approx(R.exponential_decay(step, 1e-2, 10, 0.5, staircase), rel=1e-14, abs=0.0)
    assert s(0) == 1e-2 and s(10) == pytest.approx(5e-3, rel=1e-14)
    assert s(11) == (pytest.approx(5e-3, rel=1e-14) if staircase else pytest.approx(1e-2 * 0.5 ** 1.1, rel=1e-14))
    assert s(9) == (1e-2 if staircase else pytest.approx(1e-2 * 0.5 ** 0.9, rel=1e-14))


def test_piecewise_constant_decay():
    from tf2_yolo_amd.optimizers.schedules import PiecewiseConstantDecay
    s = PiecewiseConstantDecay([3, 7], [1e-3, 1e-4, 0.0])
    want = {0: 1e-3, 1: 1e-3, 3: 1e-3, 4: 1e-4, 7: 1e-4, 8: 0.0, 1000: 0.0}     # a boundary belongs to the LEFT piece
    for step, v in want.items():
        assert s(step) == v == R.piecewise_constant(step, [3, 7], [1e-3, 1e-4, 0.0]), step
    with pytest.raises(ValueError):
        PiecewiseConstantDecay([3, 7], [1e-3, 1e-4])


@pytest.mark.parametrize("alpha", [0.0, 0.1])
def test_cosine_decay(alpha):
    from tf2_yolo_amd.optimizers.schedules import CosineDecay
    s = CosineDecay(2e-3, decay_steps=20, alpha=alpha)
    for step in (0, 1, 20, 21, 1000):
        assert s(step) == pytest.approx(R.cosine_decay(step, 2e-3, 20, alpha), rel=1e-13, abs=1e-20)
    assert s(0) == pytest.approx(2e-3, rel=1e-14)
    assert s(10) == pytest.approx(2e-3 * ((1 - alpha) * 0.5 + alpha), rel=1e-13)
    assert s(20) == s(21) == s(1000) == pytest.approx(2e-3 * alpha, rel=1e-13, abs=1e-19)


@pytest.mark.parametrize("cls", ["Adam", "SGD"])
def test_rate_of_a_step_schedule_decay_and_assignment(cls):
    """the rate a step uses: schedule(iterations before the increment) -- 0 at the first step --, the legacy
    lr / (1 + decay * iterations), and a value assigned through `learning_rate` or `lr` between steps"""
    from tf2_yolo_amd import optimizers
    from tf2_yolo_amd.optimizers.schedules import PiecewiseConstantDecay
    make = getattr(optimizers, cls)
    seen = []
    o = make(lambda step: seen.append(step) or 0.5 ** step)
    for k in range(3):
        o.iterations += 1                      # (what step() / refresh_hyper do first)
        assert o._lr_now() == 0.5 ** k
    assert seen == [0, 1, 2]
    o = make(1e-2, decay=0.25)
    for k in (0, 1, 10, 11, 1000):
        o.iterations = k + 1
        assert o._lr_now() == pytest.approx(R.legacy_decay(k, 1e-2, 0.25), rel=1e-15)
    o = make(PiecewiseConstantDecay([3], [1e-3, 0.0]), decay=1.0)
    o.iterations = 3
    assert o._lr_now() == pytest.approx(1e-3 / 3.0, rel=1e-15)
    o = make(lr=3e-4)
    assert o.learning_rate == o.lr == 3e-4
    o.lr = 1e-5
    o.iterations = 1
    assert o.learning_rate == 1e-5 and o._lr_now() == 1e-5
    o.learning_rate = 2e-5
    assert o.lr == 2e-5 and o._lr_now() == 2e-5


# ---- argument validation ----
@pytest.mark.parametrize("cls", ["Adam", "SGD"])
def test_argument_validation(cls):
    from tf2_yolo_amd import optimizers
    make = getattr(optimizers, cls)
    with pytest.raises(TypeError):
        make(1e-3, weight_decay=1e-4)                      # nothing is swallowed silently
    with pytest.raises(TypeError):
        make(1e-3, momentun=0.9)
    for a, b in (("clipnorm", "clipvalue"), ("clipnorm", "global_clipnorm"), ("clipvalue", "global_clipnorm")):
        with pytest.raises(ValueError):
            make(1e-3, **{a: 1.0, b: 1.0})
    with pytest.raises(ValueError):
        make(1e-3, clipnorm=1.0, clipvalue=1.0, global_clipnorm=1.0)
    for name in ("clipnorm", "clipvalue", "global_clipnorm"):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError):
                make(1e-3, **{name: bad})
        assert getattr(make(1e-3, **{name: 2.5}), name) == 2.5
    o = make(1e-3, name="opt")
    assert o.name == "opt" and o.clipnorm is None and o.clipvalue is None and o.global_clipnorm is None


def test_sgd_momentum_range_and_which_form_runs():
    from tf2_yolo_amd.optimizers import SGD, Adam
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SGD(1e-3, momentum=bad)
    assert SGD(1e-3, momentum=0.0).momentum == 0.0 and SGD(1e-3, momentum=1.0).momentum == 1.0
    # plain SGD stays the one eager launch; any new option makes it recordable. Adam always was.
    assert not SGD(1e-3).capturable and not SGD(1e-3, nesterov=True).capturable
    assert SGD(1e-3, momentum=0.9, nesterov=True).capturable and SGD(1e-3, clipvalue=1.0).capturable
    assert Adam(1e-3).capturable and not Adam(1e-3)._extended
    assert Adam(1e-3, amsgrad=True)._extended and Adam(1e-3, global_clipnorm=1.0)._extended
    assert Adam(1e-3).last_grad_norm() is None and SGD(1e-3, clipvalue=1.0).last_grad_norm() is None


# ---- the chunk / variable table ----
@pytest.mark.parametrize("chunk", [8192, 64, 4096])
def test_chunk_table_partitions_the_variables_and_nothing_else(chunk):
    from tf2_yolo_amd.ops import build_chunk_table
    variables, total = R.layout()
    assert [s for _, s in variables] == [1, 3, 64, 65, 4099, 70000] and all(o % 64 == 0 for o, _ in variables)
    off, ln, var, first = build_chunk_table(variables, chunk)
    assert off.dtype == np.int64 and ln.dtype == var.dtype == first.dtype == np.int32
    assert len(off) == len(ln) == len(var) == sum(math.ceil(s / chunk) for _, s in variables)
    count = np.zeros(total, dtype=np.int64)
    owner = np.full(total, -1)
    for v, (o, s) in enumerate(variables):
        owner[o:o + s] = v
    for c in range(len(off)):
        assert 0 < ln[c] <= chunk
        sl = slice(int(off[c]), int(off[c]) + int(ln[c]))
        count[sl] += 1
        assert (owner[sl] == var[c]).all()            # inside ONE variable: no straddling, no padding element
    assert (count[owner >= 0] == 1).all()             # every variable element in exactly one chunk
    assert (count[owner < 0] == 0).all()              # no padding element in any chunk
    # variable v owns the consecutive chunks first[v] .. first[v + 1] - 1, in address order
    assert first[0] == 0 and first[-1] == len(off) and len(first) == len(variables) + 1
    for v in range(len(variables)):
        mine = np.arange(first[v], first[v + 1])
        assert (var[mine] == v).all() and (np.diff(off[mine]) > 0).all()
        assert ln[mine].sum() == variables[v][1]
    assert (off % 4 == 0).all()                       # 64-aligned variables, chunk a multiple of 4: float4 loads are aligned


def test_chunk_table_of_anchor_boxes_and_bad_input():
    from tf2_yolo_amd.ops import build_chunk_table
    off, ln, var, first = build_chunk_table([(2 * i, 2) for i in range(9)])     # one variable per anchor box
    assert off.tolist() == list(range(0, 18, 2)) and set(ln.tolist()) == {2}
    assert var.tolist() == list(range(9)) and first.tolist() == list(range(10))
    with pytest.raises(ValueError):
        build_chunk_table([(0, 65), (64, 3)])         # overlapping variables
    with pytest.raises(ValueError):
        build_chunk_table([(0, 8)], chunk=6)
