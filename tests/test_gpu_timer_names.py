"""The kernel names of ops.KernelTimer (bench.py's roofline block, scripts/layer_table.py) come from the library:
every templated launcher notes the family it launches and yolo_last_conv_kernel reports it (include/yolo_hip.h).
One table of the smallest shapes that reach each dispatch branch; every literal is read off the C++ dispatch
(launch_gather_planes, launch_conv_win, launch_conv_patch, launch_wgrad_planes, launch_wgrad_win, dispatch_gather,
launch_gather_split, launch_wgrad_split, dispatch_wgrad, stem_fwd_supported) at the library's default switches.
Operands are zeros: only the dispatch is under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, PER_TAP, MFMA16 = {}, {"OPT_WGRAD_WIN": 0}, {"OPT_WGRAD_WIN": 3}

# (entry point, (N, H, W, Cin, Cout, k, stride, padding), options, expected name, expected launches)
CASES = [
    # ---- conv2d_fwd_planes ----
    ("fwd_planes", (1, 8, 8, 16, 32, 1, 1, "same"), {}, "gather_conv_planes_kernel<128,32,4,1>", 1),
    ("fwd_planes", (1, 8, 8, 16, 64, 1, 1, "same"), {}, "gather_conv_planes_kernel<128,64,4,2>", 1),
    # one 16-channel block: conv_split_parts() finds nothing to split, the 8-wave 1x1 tile stays
    ("fwd_planes", (1, 8, 8, 16, 128, 1, 1, "same"), {}, "gather_conv_planes_kernel<128,128,4,2>", 1),
    # launch_gather_planes, the block after `waves == 4`: conv_split_parts() > 1 (16 channel blocks, 2 parts) -> <128,128,2,2>
    ("fwd_planes", (1, 8, 8, 256, 128, 1, 1, "same"), {}, "gather_conv_planes_kernel<128,128,2,2>", 1),
    ("fwd_planes", (1, 8, 8, 16, 128, 3, 1, "same"), {}, "conv_win_planes_kernel<128,128>", 1),
    ("fwd_planes", (1, 8, 8, 16, 64, 3, 1, "same"), {}, "gather_conv_planes_kernel<128,64,4,2>", 1),     # 1 patch tile < 256
    ("fwd_planes", (1, 256, 256, 16, 64, 3, 1, "same"), {}, "conv_patch_planes_kernel<256,64>", 1),      # 256 patch tiles
    ("fwd_planes", (6, 80, 80, 16, 128, 3, 1, "same"), {}, "conv_patch_planes_kernel<128,128>", 1),      # rows > 64 px, 300 tiles
    ("fwd_planes", (1, 80, 80, 16, 128, 3, 1, "same"), {}, "gather_conv_planes_kernel<128,128,2,2>", 1),  # ... 50 tiles
    ("fwd_planes", (1, 8, 8, 16, 128, 3, 2, "darknet_s2"), {}, "gather_conv_planes_kernel<128,128,2,2>", 1),
    # ---- conv2d_dgrad_planes (the tile's columns are Cin) ----
    ("dgrad_planes", (1, 8, 8, 128, 32, 3, 1, "same"), {}, "conv_win_planes_kernel<128,128>", 1),   # (dgrad_impl wants Cout % 32 == 0)
    ("dgrad_planes", (1, 8, 8, 32, 64, 3, 2, "darknet_s2"), {}, "gather_conv_planes_kernel<128,32,4,1>", 1),   # four parity classes, one launch
    # ---- conv2d_wgrad_planes ----
    ("wgrad_planes", (1, 8, 8, 32, 128, 3, 1, "same"), WIN, "wgrad_win_planes_kernel<128,288>", 1),
    ("wgrad_planes", (1, 8, 8, 32, 128, 3, 1, "same"), MFMA16, "wgrad_win_planes_kernel<128,288,mfma16>", 1),
    ("wgrad_planes", (1, 8, 8, 32, 128, 3, 1, "same"), PER_TAP, "wgrad_planes_kernel<128,256,2,2>", 1),   # 288 columns, 64 pixels: the wide tile
    ("wgrad_planes", (1, 8, 8, 64, 32, 1, 1, "same"), {}, "wgrad_planes_kernel<64,64,2,2>", 1),
    ("wgrad_planes", (1, 8, 8, 16, 32, 3, 1, "same"), {}, "wgrad_planes_kernel<64,128,2,4>", 1),
    ("wgrad_planes", (1, 8, 8, 64, 128, 1, 1, "same"), {}, "wgrad_planes_kernel<128,64,4,2>", 1),
    ("wgrad_planes", (1, 8, 8, 48, 128, 3, 1, "same"), {}, "wgrad_planes_kernel<128,256,2,2>", 1),       # Cin % 32 != 0: no window kernel
    ("wgrad_planes", (1, 8, 8, 256, 128, 1, 1, "same"), {}, "wgrad_planes_kernel<128,128,2,2>", 1),
    # ---- the fp32 / bf16 entry points ----
    # stem_fwd_supported() in csrc/stem.hip: with the matrix-core stem (YOLO_STEM_MFMA, default 8) there is no pixel floor
    ("fwd", (1, 8, 8, 3, 32, 3, 1, "same"), {}, "stem_conv3x3_kernel", 1),
    ("fwd", (1, 1024, 1024, 3, 32, 3, 1, "same"), {}, "stem_conv3x3_kernel", 1),                         # 2^20 pixels
    ("fwd", (1, 8, 8, 3, 32, 3, 1, "valid"), {}, "gather_conv_kernel<128,32,flat>", 1),                  # not 'same': not the stem's
    ("fwd", (1, 8, 8, 32, 64, 3, 1, "same"), {}, "gather_conv_split_kernel<128,64,2,2>", 1),
    ("dgrad", (1, 8, 8, 32, 64, 3, 2, "darknet_s2"), {}, "gather_conv_kernel<128,32>", 4),               # one launch per parity class
    ("wgrad", (1, 8, 8, 16, 64, 3, 1, "same"), {}, "wgrad_split_kernel<64,128,2,2>", 1),
    ("wgrad", (1, 8, 8, 3, 32, 3, 1, "same"), {}, "wgrad_kernel", 1),
    ("stem_bwd", (1, 16, 16, 3, 32, 3, 1, "same"), {}, "stem_bn_bwd_wgrad_kernel", 1),
]


def _call(ops, kind, d):
    def z(*shape):
        return torch.zeros(shape, device="cuda")

    def planes(rows, c):
        return ops.split_planes(z(rows * c), rows, c)

    n_in, n_out, taps = d.N * d.H * d.W, d.N * d.Ho * d.Wo, d.kh * d.kw
    if kind == "fwd_planes":
        ops.conv2d_fwd_planes(d, planes(n_in, d.Cin), planes(d.Cout, taps * d.Cin))
    elif kind == "dgrad_planes":
        ops.conv2d_dgrad_planes(d, planes(n_out, d.Cout), planes(d.Cin, taps * d.Cout))
    elif kind == "wgrad_planes":
        ops.conv2d_wgrad_planes(d, planes(n_in, d.Cin), planes(n_out, d.Cout), z(d.Cout * taps * d.Cin))
    elif kind == "fwd":
        ops.conv2d_fwd(d, z(n_in * d.Cin), z(d.Cout * taps * d.Cin))
    elif kind == "dgrad":
        ops.conv2d_dgrad(d, z(n_out * d.Cout), z(d.Cin * taps * d.Cout))
    elif kind == "wgrad":
        ops.conv2d_wgrad(d, z(n_in * d.Cin), z(n_out * d.Cout), z(d.Cout * taps * d.Cin))
    else:
        ones, red = torch.ones(32, device="cuda"), torch.zeros((ops.BN_RED_SLOTS + 1) * 64, device="cuda", dtype=torch.float64)
        ops.stem_bn_bwd_wgrad(d, z(n_in * 3), z(n_in * 32), z(n_in * 32), ones, z(32), z(32), ones, 1, red, z(32), z(32), z(32 * 27))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2].get('OPT_WGRAD_WIN', '')}")
def test_timer_reports_the_launched_kernel(case):
    from tf2_yolo_amd import ops
    kind, (n, h, w, cin, cout, k, s, pad), options, name, launches = case
    ops.ensure_conv_workspace()
    ops.ensure_wgrad_workspace()
    d = ops.conv_desc((n, h, w, cin), cout, k, k, s, pad)
    ops.reset_options()
    for key, value in options.items():
        ops.set_option(getattr(ops, key), value)
    ops.TIMER = timer = ops.KernelTimer()
    try:
        _call(ops, kind, d)
    finally:
        ops.TIMER = None
        ops.reset_options()
    got = timer.summary()
    assert {k: v["launches"] for k, v in got.items()} == {name: launches}


def test_a_bracket_without_a_convolution_is_an_error():
    from tf2_yolo_amd import ops
    from tf2_yolo_amd._lib import YoloHipError
    x = torch.zeros(64, device="cuda")
    with pytest.raises(YoloHipError, match="no convolution"):
        ops.KernelTimer().bracket(0.0, lambda: ops.act_fwd(x, 1))
