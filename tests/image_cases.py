"""Case table and float64 NumPy oracle of the image preparation (tf2_yolo_amd/images.py, csrc/image.hip), GPU-free: nothing
here imports the library or touches a device. tests/test_images_cpu.py checks the oracle against torch's own bilinear
interpolation on the CPU and the past-the-cap case against the stream cap; tests/test_gpu_images.py runs the kernel.

The oracle restates the formulas of the kernel's contract in exact integers and float64. Per axis, for region index v, source
extent n and region extent r:

    den = 2 r;  num = clamp((2 v + 1) n - r, 0, (n - 1) den);  lo = num // den;  hi = min(lo + 1, n - 1);  f = (num % den) / den
    out = (top + fy (bot - top)) * rescale,   top = a + fx (b - a)

(half-pixel centres, no antialias: cv2 INTER_LINEAR, torch interpolate(mode="bilinear", align_corners=False)); outside the
region the output is pad_grey * rescale."""
import numpy as np

SOURCE_SIZES = [(1, 1), (1, 9), (300, 2), (5, 7), (33, 17), (97, 131), (64, 64)]
OUTPUT_SIZES = [(32, 64), (64, 64)]
RESCALES = [1 / 255, None]
PAD_GREY = 128

# Past the grid cap (the rule of past_cap_cases.py: work items in (2 cap, 3 cap], no multiple of the cap). The launcher counts
# one item per FOUR floats when W * 3 % 4 == 0: N = 6 images of 416 x 352 are 658 944 items, between one and two caps, so the
# case is N = 11 of 416 x 352: 11 * 416 * 352 * 3 / 4 = 1 208 064 items = 2.30 caps.
PAST_CAP_N, PAST_CAP_HW = 11, (416, 352)


def past_cap_items():
    h, w = PAST_CAP_HW
    assert (w * 3) % 4 == 0
    return PAST_CAP_N * h * w * 3 // 4


def source_images(seed=5):
    """one uint8 image per SOURCE_SIZES entry, in that order: packed back to back their byte offsets are 0, 3, 30, 1830,
    1935, 3618, 41739 -- odd and unaligned"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCE_SIZES]


def axis_taps(n, r):
    """(lo, hi, f) for every region index of one axis: int64, int64, float64"""
    v = np.arange(r, dtype=np.int64)
    den = 2 * r
    num = np.clip((2 * v + 1) * n - r, 0, (n - 1) * den)
    lo = num // den
    hi = np.minimum(lo + 1, n - 1)
    return lo, hi, (num % den).astype(np.float64) / den


def oracle_resize(img, rh, rw):
    """uint8 [h, w, 3] -> float64 [rh, rw, 3] in grey levels (no rescale)"""
    a = img.astype(np.float64)
    ylo, yhi, fy = axis_taps(img.shape[0], rh)
    xlo, xhi, fx = axis_taps(img.shape[1], rw)
    fx = fx[None, :, None]
    top = a[ylo][:, xlo] + fx * (a[ylo][:, xhi] - a[ylo][:, xlo])
    bot = a[yhi][:, xlo] + fx * (a[yhi][:, xhi] - a[yhi][:, xlo])
    return top + fy[:, None, None] * (bot - top)


def oracle_prepare(imgs, out_hw, geom, rescale, pad_grey=PAD_GREY):
    """float64 [N, H, W, 3] and the boolean mask [N, H, W] of the padding pixels. The pad value is the float32 product the
    contract names, so padding compares bit for bit."""
    H, W = out_hw
    s = 1.0 if rescale is None else float(rescale)
    pad = float(np.float32(pad_grey) * np.float32(s))
    out = np.full((len(imgs), H, W, 3), pad, dtype=np.float64)
    is_pad = np.ones((len(imgs), H, W), dtype=bool)
    for i, (img, (y0, x0, rh, rw)) in enumerate(zip(imgs, geom)):
        out[i, y0:y0 + rh, x0:x0 + rw] = oracle_resize(img, int(rh), int(rw)) * float(np.float32(s))
        is_pad[i, y0:y0 + rh, x0:x0 + rw] = False
    return out, is_pad
