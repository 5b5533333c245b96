"""Case tables of the "past the grid cap" tests (tests/test_gpu_loss.py, tests/test_gpu_glue_edges.py), GPU-free: shapes,
seeds and the work-item count AS THE LAUNCHER COUNTS IT. Nothing here imports the library or touches a device;
tests/test_past_cap_cases_cpu.py checks the table against the caps it reads from the sources.

Every streaming kernel caps its grid and walks the rest of its work with `i += gridDim.x * blockDim.x`:

  stream cap  stream_grid() of tf2_yolo_amd/csrc/common.hpp: 2048 workgroups x 256 threads = 524 288 work items per pass
  loss cap    yolo_loss_fwd_bwd / yolo_metrics of tf2_yolo_amd/csrc/loss.hip: 2048 workgroups x 4 waves, one cell per wave
              and pass = 8192 cells per pass
  danchor cap head_danchor_kernel of tf2_yolo_amd/csrc/elementwise.hip: 256 workgroups x 256 threads = 65 536 pixels per pass

Size rule of a "past the cap" case: the work items lie in (2 cap, 3 cap] -- some threads / waves run a first, a middle and
a last pass -- and are no multiple of the cap, so the last pass is partial. The loss has a second band, (cap, 2 cap): some
waves do two cells, some one. H != W and odd sizes wherever the op allows, so that a swapped divisor shows."""
from collections import namedtuple

STREAM_WORKGROUPS, STREAM_BLOCK = 2048, 256
STREAM_CAP = STREAM_WORKGROUPS * STREAM_BLOCK          # 524 288 work items per pass
LOSS_WORKGROUPS, LOSS_WAVES = 2048, 4
LOSS_CAP = LOSS_WORKGROUPS * LOSS_WAVES                # 8192 cells per pass
DANCHOR_CAP = 256 * 256                                # 65 536 pixels per pass

ANCH9 = [[0.89663461, 0.78365384], [0.375, 0.47596153], [0.27884615, 0.21634615], [0.14182692, 0.28605769],
         [0.14903846, 0.10817307], [0.07211538, 0.14663461], [0.07932692, 0.05528846], [0.03846153, 0.07211538],
         [0.02403846, 0.03125]]
ANCH5 = [[0.75, 0.70], [0.60, 0.27], [0.25, 0.42], [0.14, 0.15], [0.04, 0.05]]

# ---- loss / metrics ------------------------------------------------------------------------------------------------
# band 3: cells in (2 cap, 3 cap]; band 2: cells in (cap, 2 cap). kw: keyword arguments shared by ops.make_loss_cfg and
# the oracle's wrap_yolo_loss_vN (truth_thresh only; the loss weights are set by the tests).
LossCase = namedtuple("LossCase", "name version N g A C anchors seed band kw")

LOSS_CASES = [
    LossCase("v3-c3", 3, 7, (52, 52), 3, 3, ANCH9[:3], 1, 3, {}),                  # one 64-channel chunk (PD = 24)
    LossCase("v3-c80", 3, 4, (52, 52), 3, 80, ANCH9[:3], 1, 2, {}),                # PD = 255: all four chunks
    LossCase("v3-52x40", 3, 9, (52, 40), 3, 6, ANCH9[3:6], 2, 3, {}),              # non-square: 2080 cells per image
    LossCase("v2", 2, 7, (52, 52), 5, 20, ANCH5, 1, 3, {}),
    LossCase("v4", 4, 7, (52, 52), 3, 5, ANCH9[:3], 1, 3, {"truth_thresh": 0.7}),
    LossCase("v1", 1, 101, (14, 12), 2, 3, None, 1, 3, {}),                        # no prefetch loader, the same stride loop
    LossCase("v3-c91", 3, 8, (52, 40), 3, 91, ANCH9[:3], 2, 3, {}),                # PD = 288 > 256: the chunk-ahead loader
]
LOSS_BY_NAME = {c.name: c for c in LOSS_CASES}
# run a second time under ops.set_option(8, 8), which keeps the chunk-ahead loader for every shape
LOSS_CHUNK_AHEAD = ["v3-c3", "v2", "v4", "v3-c91"]
LOSS_GRAD_SCALE = "v3-c3"            # grad_scale = 0.5
LOSS_NO_GRAD = ["v3-c80", "v4"]      # want_grad = False
METRICS_CASES = ["v1", "v2", "v3-c3", "v4"]


def loss_cells(c):
    return c.N * c.g[0] * c.g[1]


def loss_pred_channels(c):
    return 5 * c.A + c.C if c.version == 1 else c.A * (5 + c.C)


def loss_inputs(c):
    """(y_true, y_pred) float32 arrays of a LossCase, from tests/test_gpu_loss.py::make_case (imports without a GPU)"""
    from test_gpu_loss import make_case
    yt, yp = make_case(c.N, c.g, c.A, c.C, c.anchors, c.seed, v1=c.version == 1, obj_frac=0.4 if c.version == 1 else 0.15)
    if c.version == 2:                       # softmax-like class predictions, as test_v2_loss makes them
        ypr = yp.reshape(c.N, c.g[0], c.g[1], c.A, 5 + c.C)
        ypr[..., 5:] /= ypr[..., 5:].sum(-1, keepdims=True)
    return yt, yp


def loss_case_ious(case, dtype, inputs=None):
    """OL.cal_iou of every (cell, anchor) of a case, evaluated in `dtype` on the CPU: [cells, A]. inputs: (y_true, y_pred)
    of the case's shape where they are not loss_inputs(case) (tests/saturation_cases.py)"""
    import torch
    from oracle import losses as OL
    yt, yp = loss_inputs(case) if inputs is None else inputs
    gh, gw = case.g
    t = torch.tensor(yt).to(dtype)
    p = torch.tensor(yp).to(dtype)
    if case.version == 1:
        t4 = t[..., :5].reshape(-1, gh, gw, 1, 5)
        p4 = p[..., :5 * case.A].reshape(-1, gh, gw, case.A, 5)
    else:
        t4 = t.reshape(-1, gh, gw, 1, 5 + case.C)
        p4 = p.reshape(-1, gh, gw, case.A, 5 + case.C)
    return OL.cal_iou(t4[..., :4], p4[..., :4], (gh, gw)).reshape(-1, case.A), t[..., 4].reshape(-1)


def decisions_of(iou, ignore_thresh, truth_thresh):
    """what yolo_loss_fwd_bwd exports per cell, from the IoUs [cells, A]: [0] the first maximal anchor, [1] bit b = IoU_b <
    ignore_thresh, bit 16 + b = IoU_b > truth_thresh"""
    import torch
    A = iou.shape[1]
    w = (1 << torch.arange(A)).long()
    ign = ((iou < ignore_thresh).long() * w).sum(1)
    tru = ((iou > truth_thresh).long() * w).sum(1)
    return torch.stack([torch.argmax(iou, dim=1), ign | (tru << 16)], dim=1)


# ---- glue kernels ----------------------------------------------------------------------------------------------------
# d: the shape parameters the test reads by name; items: the launcher's work-item count; cap: the cap it is measured by
GlueCase = namedtuple("GlueCase", "name d items cap")


def _g(name, items, cap=STREAM_CAP, **d):
    return GlueCase(name, d, int(items), cap)


_P_VEC, _P_SCALAR = 3 * 151 * 147, 180001              # pixels of the copy cases (66 591, odd)

GLUE_CASES = [
    # copy_channels_in: P Csrc / 4 vectorised, P Csrc scalar (C % 4 != 0 or c_off % 4 != 0)
    _g("copy_in_vec", _P_VEC * 68 // 4, P=_P_VEC, Csrc=68, Cdst=100, c_off=16),
    _g("copy_in_scalar", _P_SCALAR * 6, P=_P_SCALAR, Csrc=6, Cdst=22, c_off=3),
    # copy_channels_out: P Cdst / 4 vectorised, P Cdst scalar; the slice at the start, middle and end of the source
    _g("copy_out_vec", _P_VEC * 68 // 4, P=_P_VEC, Csrc=100, Cdst=68, c_offs=(0, 16, 32)),
    _g("copy_out_scalar", _P_SCALAR * 6, P=_P_SCALAR, Csrc=22, Cdst=6, c_offs=(0, 3, 16)),
    # upsample2x_fwd: N 2H 2W C / 4 (one thread per OUTPUT float4); upsample2x_bwd: N H W C / 4 (per INPUT float4)
    _g("upsample_fwd", 3 * 150 * 134 * 72 // 4, N=3, H=75, W=67, C=72, Cy=80, c_offs=(0, 4, 8)),
    _g("upsample_bwd", 3 * 75 * 67 * 280 // 4, N=3, H=75, W=67, C=280, Cy=288, c_offs=(0, 4, 8)),
    # space_to_depth2: N H W C (one thread per input float)
    _g("s2d", 3 * 150 * 134 * 18, N=3, H=150, W=134, C=18, Cy=80, c_off=5),
    # general max-pool: N Ho Wo C. k=5: C % 8 == 0 and H W = 5025 > 1024, so the plane kernel declines
    _g("pool_2x2s2_valid_odd", 2 * 75 * 67 * 108, N=2, H=151, W=135, C=108, k=2, s=2, pad="valid", Cy=112, c_off=4),
    _g("pool_2x2s1_same", 2 * 75 * 67 * 108, N=2, H=75, W=67, C=108, k=2, s=1, pad="same", Cy=116, c_off=3),
    _g("pool_5x5s1_same", 2 * 75 * 67 * 112, N=2, H=75, W=67, C=112, k=5, s=1, pad="same", Cy=120, c_off=8),
    # 2x2 / stride-2 fast path (and maxpool2x2_bwd): N Ho Wo C / 4
    _g("pool2x2_fast", 2 * 75 * 67 * 420 // 4, N=2, H=150, W=134, C=420),
    # bn_act_maxpool2x2_fwd: rows C / 8, rows = the pooled pixels rounded up to 16 (+ 16 zero rows with planes)
    _g("bn_act_pool", (3 * 101 * 93 + 15) // 16 * 16 * (304 // 8), N=3, H=202, W=186, C=304),
    _g("bn_act_pool_planes", ((3 * 101 * 93 + 15) // 16 + 1) * 16 * (304 // 8), N=3, H=202, W=186, C=304),
    # act_fwd / act_bwd, fill, sgd_step: n ; axpy, adam_step, adam_step_dev: n / 4 + 1
    _g("act", 1100003, n=1100003),
    _g("fill", 1100003, n=1100003),
    _g("axpy_r0", 4400000 // 4 + 1, n=4400000),
    _g("axpy_r1", 4400001 // 4 + 1, n=4400001),
    _g("axpy_r3", 4400003 // 4 + 1, n=4400003),
    _g("sgd", 1100003, n=1100003),
    _g("adam", 4400003 // 4 + 1, n=4400003),
    # head activations: P A (5 + C) pointwise (v2 / v3 / v4), P 5 A sigmoids (v1), P A softmax groups (v2)
    _g("head_v3", 52001 * 3 * 7, version=3, P=52001, A=3, C=2),
    _g("head_v4", 52001 * 3 * 7, version=4, P=52001, A=3, C=2),
    _g("head_v2", 27001 * 5 * 8, version=2, P=27001, A=5, C=3),
    _g("head_v2_softmax", 220001 * 5, version=2, P=220001, A=5, C=2),
    _g("head_v1", 110001 * 5 * 2, version=1, P=110001, A=2, C=2),
    _g("head_v4_danchors", 150001, DANCHOR_CAP, version=4, P=150001, A=3, C=2),
    # bn_act_fwd / bn_act_bwd with C % 8 == 4: P C / 4
    _g("bn_c12", 360001 * 12 // 4, P=360001, C=12),
    _g("bn_c20", 216001 * 20 // 4, P=216001, C=20),
    # down2xlabel: N (gh / 2) (gw / 2) ch ; cal_iou: the elements of the broadcast shape
    _g("down2xlabel", 4 * 58 * 54 * 85, N=4, gh=116, gw=108, ch=85),
    _g("cal_iou", 1031 * 1061, M=1031, K=1061),
]
GLUE = {c.name: c for c in GLUE_CASES}
