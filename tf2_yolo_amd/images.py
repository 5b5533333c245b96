"""Raw pixels in, network input out: the device-side half of a data reader.

`prepare` takes decoded images as they are -- uint8 RGB, any sizes -- packs them into a reused pinned staging buffer, sends
them to the device in ONE copy (a quarter of the bytes of a float32 array) and lets csrc/image.hip resize, pad and rescale
the whole batch in one launch. `letterbox_geometry` / `unletterbox` are the integer geometry of an aspect-preserving fit and
the map of detection rows back onto the original image. Resampling is bilinear with half-pixel centres and NO antialias
(cv2.resize INTER_LINEAR, the reference's reader="cv"; torch interpolate(align_corners=False)): shrinking by more than about
2x aliases, as cv2 does; PIL's resize antialiases and is not matched. File decoding stays with the caller.

Everything up to `_Plan` is host arithmetic and validation: no device is touched before the arguments are known to be good.
"""
import threading

import numpy as np
import torch

MAX_SRC, MAX_DST = 16384, 4096        # YOLO_IMAGE_MAX_SRC / YOLO_IMAGE_MAX_DST of include/yolo_hip.h
ENTRY_BYTES = 32                      # one table entry: int64 off; int32 sh, sw, y0, x0, rh, rw
ENTRY = np.dtype([("off", "<i8"), ("sh", "<i4"), ("sw", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("rh", "<i4"), ("rw", "<i4")])
assert ENTRY.itemsize == ENTRY_BYTES
RESIZE_MODES = (None, "stretch", "letterbox")


# ---- geometry (pure integer host code) --------------------------------------------------------------------------------
def stretch_geometry(src_hw, dst_hw):
    """the region is the whole output"""
    return (0, 0, int(dst_hw[0]), int(dst_hw[1]))


def letterbox_geometry(src_hw, dst_hw):
    """(y0, x0, rh, rw): the largest centred region of the output with the source's aspect ratio (the short side rounded to
    the nearest pixel, at least 1)"""
    sh, sw = int(src_hw[0]), int(src_hw[1])
    H, W = int(dst_hw[0]), int(dst_hw[1])
    if sh <= 0 or sw <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"letterbox_geometry: sizes must be positive, got {src_hw} -> {dst_hw}")
    if sh * W >= sw * H:
        rh, rw = H, max(1, (2 * sw * H + sh) // (2 * sh))
    else:
        rh, rw = max(1, (2 * sh * W + sw) // (2 * sw)), W
    return ((H - rh) // 2, (W - rw) // 2, rh, rw)


def unletterbox(rows, geom_i, dst_hw):
    """Detection rows (n, 7) float64 with x, y, w, h normalised to the network input -> the same boxes normalised to the
    ORIGINAL image that `geom_i` = (y0, x0, rh, rw) placed inside the dst_hw input. float64 on the host, nothing is clipped;
    the identity (and skipped) for stretch geometry."""
    H, W = int(dst_hw[0]), int(dst_hw[1])
    y0, x0, rh, rw = (int(v) for v in geom_i)
    rows = np.asarray(rows, dtype=np.float64)
    if (y0, x0, rh, rw) == (0, 0, H, W) or rows.shape[0] == 0:
        return rows
    out = rows.copy()
    out[:, 0] = (rows[:, 0] * W - x0) / rw
    out[:, 1] = (rows[:, 1] * H - y0) / rh
    out[:, 2] = rows[:, 2] * W / rw
    out[:, 3] = rows[:, 3] * H / rh
    return out


def work_items(n, h, w, vec=None):
    """work items of one launch as yolo_image_prepare counts them: one per four floats when W * 3 % 4 == 0 (the output of
    `prepare` is always 16-byte aligned), else one per float"""
    floats = n * h * w * 3
    if vec is None:
        vec = (w * 3) % 4 == 0
    return floats // 4 if vec else floats


# ---- validation --------------------------------------------------------------------------------------------------------
class _Plan:
    """what `prepare` found in its arguments: kind "host" (list of uint8 arrays [h, w, 3]) or "cuda" (one uint8 tensor
    [N, h, w, 3]), geom int32 [N, 4], the packed table and the byte count of the packed pixels"""
    __slots__ = ("kind", "items", "n", "hw", "geom", "table", "src_bytes", "rescale", "pad_grey")


def _check_image(a, what):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise TypeError(f"{what} must be a uint8 ndarray, got {type(a).__name__}"
                        + (f" of {a.dtype}" if isinstance(a, np.ndarray) else ""))
    if a.ndim != 3 or a.shape[2] != 3:
        raise TypeError(f"{what} must have the shape [h, w, 3], got {tuple(a.shape)}")
    if min(a.shape[:2]) < 1 or max(a.shape[:2]) > MAX_SRC:
        raise ValueError(f"{what}: sides must be in 1..{MAX_SRC}, got {a.shape[0]} x {a.shape[1]}")


def check_batch(x, hw=None):
    """x as the training calls take it with rescale=: a uint8 batch [n, H, W, 3] (ndarray or tensor) already at the
    network's size hw (None: any one size); returns x"""
    if not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
        raise TypeError(f"with rescale= the images must be a uint8 array [N, H, W, 3], got {type(x).__name__}")
    if x.dtype not in (np.uint8, torch.uint8):
        raise TypeError(f"with rescale= the images must be uint8, got {x.dtype}")
    if len(x.shape) != 4 or x.shape[3] != 3:
        raise TypeError(f"a batch of images must have the shape [N, H, W, 3], got {tuple(x.shape)}")
    if hw is not None and tuple(x.shape[1:3]) != tuple(hw):
        raise ValueError(f"the images are {x.shape[1]} x {x.shape[2]} but the network input is {hw[0]} x {hw[1]}: training "
                         f"does not resize (labels are tied to the geometry)")
    return x


def plan(images, size_hw, rescale=1 / 255, resize="stretch", pad_grey=128):
    """validate the arguments of `prepare` and lay the batch out; touches no device"""
    if resize not in RESIZE_MODES:
        raise ValueError(f"resize must be None, 'stretch' or 'letterbox', got {resize!r}")
    H, W = int(size_hw[0]), int(size_hw[1])
    if not (1 <= H <= MAX_DST and 1 <= W <= MAX_DST):
        raise ValueError(f"the output sides must be in 1..{MAX_DST}, got {H} x {W}")
    p = _Plan()
    p.rescale = 1.0 if rescale is None else float(rescale)
    p.pad_grey = float(pad_grey)
    if not np.isfinite(p.rescale) or not np.isfinite(p.pad_grey):
        raise ValueError(f"rescale and pad_grey must be finite, got {rescale!r}, {pad_grey!r}")
    if torch.is_tensor(images) and not images.is_cuda:
        images = images.detach().numpy()
    if torch.is_tensor(images):
        if images.dtype != torch.uint8:
            raise TypeError(f"images must be uint8, got a tensor of {images.dtype}")
        if images.dim() != 4 or images.shape[3] != 3:
            raise TypeError(f"a batch of images must have the shape [N, h, w, 3], got {tuple(images.shape)}")
        p.kind, p.items, sizes = "cuda", images, [tuple(images.shape[1:3])] * images.shape[0]
    elif isinstance(images, np.ndarray):
        if images.dtype != np.uint8:
            raise TypeError(f"images must be uint8, got an ndarray of {images.dtype}")
        if images.ndim != 4 or images.shape[3] != 3:
            raise TypeError(f"a batch of images must have the shape [N, h, w, 3], got {tuple(images.shape)}")
        p.kind, p.items, sizes = "host", images, [tuple(images.shape[1:3])] * images.shape[0]
    elif isinstance(images, (list, tuple)):
        for i, a in enumerate(images):
            _check_image(a, f"images[{i}]")
        p.kind, p.items, sizes = "host", list(images), [tuple(a.shape[:2]) for a in images]
    else:
        raise TypeError(f"images must be a uint8 ndarray [N, h, w, 3], a list of uint8 ndarrays [h, w, 3] or a CUDA uint8 "
                        f"tensor, got {type(images).__name__}")
    p.n, p.hw = len(sizes), (H, W)
    if p.n == 0:
        raise ValueError("no images")
    if p.n * H * W * 3 >= 2 ** 31:
        raise ValueError(f"{p.n} images of {H} x {W} are more than 2^31 values: prepare them in smaller batches")
    for i, (h, w) in enumerate(sizes[:1] if not isinstance(p.items, list) else sizes):
        if not (1 <= h <= MAX_SRC and 1 <= w <= MAX_SRC):
            raise ValueError(f"images[{i}]: sides must be in 1..{MAX_SRC}, got {h} x {w}")
        if resize is None and (h, w) != (H, W):
            raise ValueError(f"images[{i}] is {h} x {w} but the network input is {H} x {W}: pass resize='stretch' or "
                             f"resize='letterbox'")
    geo = letterbox_geometry if resize == "letterbox" else stretch_geometry
    p.geom = np.array([geo(s, (H, W)) for s in sizes], dtype=np.int32).reshape(p.n, 4)
    p.table, p.src_bytes = pack_table(sizes, p.geom)
    return p


def pack_table(sizes, geom):
    """the device table of images packed one after another: (structured array of ENTRY, total bytes of the pixels)"""
    t = np.zeros(len(sizes), dtype=ENTRY)
    nbytes = np.array([h * w * 3 for h, w in sizes], dtype=np.int64)
    t["off"] = np.cumsum(nbytes) - nbytes
    t["sh"], t["sw"] = [s[0] for s in sizes], [s[1] for s in sizes]
    g = np.asarray(geom, dtype=np.int32).reshape(len(sizes), 4)
    t["y0"], t["x0"], t["rh"], t["rw"] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    return t, int(nbytes.sum())


# ---- device side -------------------------------------------------------------------------------------------------------
def _round_up(n, k):
    return (n + k - 1) // k * k


class _Staging:
    """one pinned uint8 buffer, grown when needed and reused by every call: [table | pixels]. The event of the last copy out
    of it is waited for before the host writes it again."""

    def __init__(self):
        self.buf = None
        self.host = None
        self.copied = None
        self.lock = threading.Lock()

    def reserve(self, nbytes):
        if self.copied is not None:
            self.copied.synchronize()
            self.copied = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(_round_up(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
            self.host = self.buf.numpy()
        return self.host


_STAGING = _Staging()
_TABLES = {}     # (device, h, w, geometry) -> device table of equal-size images packed back to back, any batch up to its length


def _same_size_table(device, n, hw, geom):
    """device table for n images of one size packed back to back (a CUDA tensor [N, h, w, 3]; the feeder's uint8 batches):
    entry i does not depend on n, so one table per (size, geometry) serves every batch up to its length. Built once, with
    one small copy; later calls copy nothing."""
    key = (str(device), hw, tuple(int(v) for v in geom))
    t = _TABLES.get(key)
    if t is None or t.shape[0] < n * ENTRY_BYTES:
        cap = max(64, n)
        host, _ = pack_table([hw] * cap, np.tile(np.asarray(geom, dtype=np.int32), (cap, 1)))
        t = _TABLES[key] = torch.from_numpy(host.view(np.uint8).copy()).to(device)
    return t


def rescale_on_device(x_u8, out, rescale=1 / 255, geom=None, pad_grey=128):
    """uint8 CUDA tensor [N, h, w, 3] -> float32 `out` [N, H, W, 3] on the current stream, no host copy: every image into
    the region `geom` (default: the whole output). Equal sizes give exactly float32(x) * float32(rescale)."""
    from . import ops
    n, h, w = int(x_u8.shape[0]), int(x_u8.shape[1]), int(x_u8.shape[2])
    H, W = int(out.shape[1]), int(out.shape[2])
    g = stretch_geometry((h, w), (H, W)) if geom is None else geom
    if not x_u8.is_contiguous():
        x_u8 = x_u8.contiguous()
    ops.image_prepare(x_u8, n * h * w * 3, _same_size_table(x_u8.device, n, (h, w), g), n, out,
                      1.0 if rescale is None else float(rescale), pad_grey)
    return out


def prepare(images, size_hw, rescale=1 / 255, resize="stretch", pad_grey=128, out=None):
    """images: uint8 ndarray [N, h, w, 3], list / tuple of uint8 ndarrays [h_i, w_i, 3], or CUDA uint8 tensor [N, h, w, 3]
    -> (x, geom): x float32 CUDA [N, H, W, 3] (`out` if given), geom int32 ndarray [N, 4] = (y0, x0, rh, rw) per image.
    resize: None (every image must already be size_hw), "stretch" or "letterbox" (aspect kept, centred, the rest
    float32(pad_grey) * float32(rescale)). rescale None = 1.0. One non-blocking H2D copy on the current stream, one launch."""
    from . import ops
    p = plan(images, size_hw, rescale=rescale, resize=resize, pad_grey=pad_grey)
    H, W = p.hw
    if out is not None:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                and tuple(out.shape) == (p.n, H, W, 3)):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of shape {(p.n, H, W, 3)}")
    if p.kind == "cuda":
        if out is None:
            out = torch.empty((p.n, H, W, 3), dtype=torch.float32, device=p.items.device)
        rescale_on_device(p.items, out, p.rescale, tuple(p.geom[0]), p.pad_grey)
        return out, p.geom
    if out is None:
        out = torch.empty((p.n, H, W, 3), dtype=torch.float32, device="cuda")
    head = _round_up(p.n * ENTRY_BYTES, 256)
    total = head + p.src_bytes
    with _STAGING.lock:
        host = _STAGING.reserve(total)
        host[:p.n * ENTRY_BYTES] = p.table.view(np.uint8)
        if isinstance(p.items, np.ndarray):
            np.copyto(host[head:total].reshape(p.items.shape), p.items)
        else:
            for a, off in zip(p.items, p.table["off"]):
                np.copyto(host[head + int(off):head + int(off) + a.size].reshape(a.shape), a)
        dev = torch.empty(total, dtype=torch.uint8, device=out.device)
        dev.copy_(_STAGING.buf[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(out.device))
        _STAGING.copied = ev
    ops.image_prepare(dev[head:], p.src_bytes, dev, p.n, out, p.rescale, p.pad_grey)
    return out, p.geom
