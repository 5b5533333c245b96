"""Host side of the image preparation (tf2_yolo_amd/images.py) and the oracle of tests/image_cases.py, without a device."""
import numpy as np
import pytest
import torch

import image_cases as IC
from tf2_yolo_amd import images


@pytest.mark.parametrize("out_hw", IC.OUTPUT_SIZES + [(7, 3)])
def test_oracle_agrees_with_torch_bilinear(out_hw):
    """stretch = torch.nn.functional.interpolate(float64, bilinear, align_corners=False, antialias=False) to 1e-9 grey levels"""
    worst = 0.0
    for img in IC.source_images() + [np.random.default_rng(9).integers(0, 256, (416, 416, 3), dtype=np.uint8)]:
        got = IC.oracle_resize(img, *out_hw)
        t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(t, size=out_hw, mode="bilinear", align_corners=False, antialias=False)
        worst = max(worst, float(np.abs(got - ref[0].permute(1, 2, 0).numpy()).max()))
    print(f"oracle vs torch, output {out_hw}: worst difference {worst:.3g} grey levels")
    assert worst <= 1e-9


def test_oracle_equal_size_is_the_input():
    for img in IC.source_images():
        assert np.array_equal(IC.oracle_resize(img, *img.shape[:2]), img.astype(np.float64))
    lo, hi, f = IC.axis_taps(97, 97)
    assert np.array_equal(lo, np.arange(97)) and not f.any()


@pytest.mark.parametrize("dst", IC.OUTPUT_SIZES + [(416, 416), (7, 3), (1, 1)])
def test_letterbox_geometry_properties(dst):
    H, W = dst
    for sh, sw in IC.SOURCE_SIZES + [(416, 416), (480, 640), (1080, 1920), (16384, 1), (1, 16384), (3, 4)]:
        y0, x0, rh, rw = images.letterbox_geometry((sh, sw), dst)
        assert 1 <= rh <= H and 1 <= rw <= W and y0 >= 0 and x0 >= 0 and y0 + rh <= H and x0 + rw <= W     # fits
        assert rh == H or rw == W                                                                        # one side is full
        assert y0 == (H - rh) // 2 and x0 == (W - rw) // 2 and (H - rh) - 2 * y0 in (0, 1) and (W - rw) - 2 * x0 in (0, 1)
        # the aspect ratio is kept within one pixel of the free side (or that side is the 1-pixel minimum)
        if rh == H:
            assert abs(rw - sw * H / sh) <= 1 or rw == 1 or rw == W
        if rw == W:
            assert abs(rh - sh * W / sw) <= 1 or rh == 1 or rh == H
    assert images.stretch_geometry((5, 7), dst) == (0, 0, H, W)
    assert images.letterbox_geometry(dst, dst) == (0, 0, H, W)


def test_unletterbox_inverts_the_forward_map():
    rng = np.random.default_rng(3)
    for (sh, sw), dst in [((33, 17), (64, 64)), ((97, 131), (32, 64)), ((300, 2), (64, 64)), ((480, 640), (416, 416))]:
        H, W = dst
        y0, x0, rh, rw = g = images.letterbox_geometry((sh, sw), dst)
        # boxes relative to the original image, as corners; the forward map places them in the network input
        c = rng.random((50, 2, 2))                       # [box, corner, (x, y)] in [0, 1)
        lo, hi = c.min(1), c.max(1)
        fwd = lambda p: np.stack([(p[:, 0] * rw + x0) / W, (p[:, 1] * rh + y0) / H], axis=1)
        flo, fhi = fwd(lo), fwd(hi)
        rows = np.zeros((50, 7))
        rows[:, 0:2], rows[:, 2:4], rows[:, 4:] = (flo + fhi) / 2, fhi - flo, rng.random((50, 3))
        back = images.unletterbox(rows, g, dst)
        assert back.dtype == np.float64 and back is not rows
        assert np.abs(back[:, 0:2] - back[:, 2:4] / 2 - lo).max() <= 1e-12
        assert np.abs(back[:, 0:2] + back[:, 2:4] / 2 - hi).max() <= 1e-12
        assert np.array_equal(back[:, 4:], rows[:, 4:])
    rows = rng.random((4, 7))
    assert images.unletterbox(rows, (0, 0, 64, 32), (64, 32)) is rows                  # stretch geometry: skipped
    far = np.array([[1.5, -0.5, 3.0, 2.0, 1, 0, 1]])
    out = images.unletterbox(far, (16, 0, 32, 64), (64, 64))
    assert np.array_equal(out[0, :4], [1.5, (-0.5 * 64 - 16) / 32, 3.0, 4.0])          # nothing is clipped
    assert images.unletterbox(np.zeros((0, 7)), (16, 0, 32, 64), (64, 64)).shape == (0, 7)


def test_prepare_refuses_bad_arguments_before_the_device():
    u8 = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    for bad in (u8.astype(np.float32), u8.astype(np.int32), torch.zeros(2, 8, 8, 3),      # not uint8
                u8[0], u8[..., :1], np.zeros((2, 8, 8, 4), np.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8),   # rank, channels
                [u8[0], u8[0].astype(np.float32)], [u8[0], u8[0, :, :, 0]], [u8], [[1, 2, 3]], "images", 5, None):
        with pytest.raises(TypeError):
            images.prepare(bad, (8, 8))
    with pytest.raises(ValueError, match="resize"):
        images.prepare(u8, (8, 8), resize="bicubic")
    with pytest.raises(ValueError, match="8 x 8.*16 x 8|16 x 8.*8 x 8"):
        images.prepare(u8, (16, 8), resize=None)
    with pytest.raises(ValueError, match="5 x 7"):
        images.prepare([u8[0], np.zeros((5, 7, 3), np.uint8)], (8, 8), resize=None)
    with pytest.raises(ValueError, match="no images"):
        images.prepare([], (8, 8))
    with pytest.raises(ValueError, match="4096"):
        images.prepare(u8, (4097, 8))
    with pytest.raises(ValueError, match="16384"):
        images.prepare([np.zeros((1, 16385, 3), np.uint8)], (8, 8))
    with pytest.raises(ValueError, match="2\\^31"):
        images.prepare(np.zeros((43, 1, 1, 3), np.uint8), (4096, 4096))
    with pytest.raises(ValueError, match="finite"):
        images.prepare(u8, (8, 8), rescale=float("nan"))
    with pytest.raises(TypeError, match="uint8"):
        images.check_batch(u8.astype(np.float32), (8, 8))
    with pytest.raises(ValueError, match="does not resize"):
        images.check_batch(u8, (16, 16))


def test_plan_packs_the_table_the_kernel_reads():
    imgs = IC.source_images()
    p = images.plan(imgs, (32, 64), rescale=None, resize="letterbox")
    assert p.rescale == 1.0 and p.table.dtype.itemsize == 32 and p.geom.dtype == np.int32 and p.geom.shape == (len(imgs), 4)
    assert p.table["off"].tolist() == [0, 3, 30, 1830, 1935, 3618, 41739] and p.src_bytes == 41739 + 64 * 64 * 3
    assert [tuple(r) for r in p.geom] == [images.letterbox_geometry(s, (32, 64)) for s in IC.SOURCE_SIZES]
    raw = p.table.view(np.uint8).reshape(len(imgs), 32)
    assert raw[3, :8].view("<i8")[0] == 1830 and raw[3, 8:].view("<i4").tolist() == [5, 7, *p.geom[3]]
    q = images.plan(np.zeros((3, 64, 64, 3), np.uint8), (64, 64), resize=None)
    assert q.table["off"].tolist() == [0, 12288, 24576] and [tuple(r) for r in q.geom] == [(0, 0, 64, 64)] * 3


def test_past_cap_case_is_past_the_stream_cap():
    from past_cap_cases import STREAM_CAP
    items = IC.past_cap_items()
    assert items == images.work_items(IC.PAST_CAP_N, *IC.PAST_CAP_HW)
    assert 2 * STREAM_CAP < items <= 3 * STREAM_CAP and items % STREAM_CAP != 0
    assert STREAM_CAP < images.work_items(6, 416, 352) < 2 * STREAM_CAP        # (the size that is NOT past the cap twice)


def test_detect_images_signature():
    """detect keeps its signature (float32 network input); detect_images is detect on raw pixels: the three preparation
    keywords first, off by default, then detect's own arguments with detect's defaults"""
    import inspect
    from tf2_yolo_amd.model import Model
    d = inspect.signature(Model.detect).parameters
    r = inspect.signature(Model.detect_images).parameters
    assert list(r)[:5] == ["self", "x", "rescale", "resize", "pad_grey"] and set(r) - set(d) == {"rescale", "resize", "pad_grey"}
    assert (r["rescale"].default, r["resize"].default, r["pad_grey"].default) == (None, None, 128)
    assert all(r[k].default == d[k].default for k in d if k not in ("self", "x"))
    for name in ("predict",):
        p = inspect.signature(getattr(Model, name)).parameters
        assert (p["rescale"].default, p["resize"].default, p["pad_grey"].default) == (None, None, 128)
    for name in ("fit", "evaluate", "train_on_batch", "test_on_batch"):
        assert inspect.signature(getattr(Model, name)).parameters["rescale"].default is None
