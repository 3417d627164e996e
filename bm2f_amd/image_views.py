"""The reference's input pipeline on the device, bit for bit: PIL resize, crop, flip, normalise, pad and stack.

The reference's mappers (``mask2former/data/dataset_mappers``, ``mask2former_video/data_video/augmentation.py``,
detectron2's ``DatasetMapper`` / ``DatasetMapperTTA``) resize the uint8 image on the host with PIL
(``ResizeTransform`` -> ``Image.resize(BILINEAR)``, ``NEAREST`` for label maps and masks); the model then computes
``(x - pixel_mean) / pixel_std`` and ``ImageList.from_tensors(..., size_divisibility)``.  Pillow's 8-bit resize is
integer arithmetic, restated here exactly (``bilinear_table``, ``nearest_table``; Pillow ``Resample.c`` and
``Geometry.c``), so the target is equality with PIL, not closeness.  ``m2f_image_views`` and ``m2f_label_views``
(``csrc/image_views.hip``) run all views of a call in one launch from one uploaded table.

On CPU tensors the same definitions run in numpy / torch, so the semantics are testable without a GPU.  That path
is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.

Oracles: the restatement was run against Pillow (tests/test_image_views_cpu.py does so live, and
tests/golden/image_views.npz records Pillow's outputs for machines without it).  The size helpers
(:func:`resize_shortest_edge_size`, :func:`lsj_view`) restate detectron2's ``ResizeShortestEdge``, ``ResizeScale``
and ``FixedSizeCrop``; detectron2 is not installed where this was written and they have not been run against it.

Colour: a :class:`View` may carry a :class:`bm2f_amd.color_aug.ColorAug` (``ColorAugSSDTransform`` or the video
mappers' brightness / contrast / saturation blends, defined in :mod:`bm2f_amd.color_aug`).  The operations run inside
the same kernel (``m2f_image_views_color``) on the pixels that show the image, never on fill or pad; a contrast blend
costs one more launch before it (``m2f_image_views_sum``, the view's exact integer sum; the host never reads it).
With every ``color`` left None the call is ``m2f_image_views`` exactly as before.  The colour definitions have not
been run against cv2 or detectron2.

Instance annotations (RLE, arrays and polygons) under the same views are :mod:`bm2f_amd.instance_views` and
:mod:`bm2f_amd.instance_mappers`.  Out of scope: reading files, rotation (``cv2.warpAffine``), source-space
``T.RandomCrop`` of the video mappers, the retry loop of ``RandomCrop_CategoryAreaConstraint`` (pass the chosen window
as ``View.crop``) and the resize of float images (detectron2 uses ``F.interpolate`` there, not PIL).
"""
from __future__ import annotations

import copy
import ctypes
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _native
from . import color_aug as _ca
from .label_planes import LABEL_DTYPES
from .tta import tta_view_sizes

_FIELDS = 20          # include/bm2f.h: M2F_VIEW_FIELDS
MAX_KSIZE = 131       # include/bm2f.h: M2F_VIEW_MAX_KSIZE: a down-scale of at most 65x per axis
_PRECISION_BITS = 22  # Pillow Resample.c: PRECISION_BITS = 32 - 8 - 2
_U8 = 3               # include/bm2f.h: M2F_U8


@dataclasses.dataclass(frozen=True)
class View:
    """One output view of a source image (or of a source's label planes).

    size: the resized (h, w).  source: index into the call's list of sources.  crop: (y0, x0, h, w) in resized
    coordinates, default the whole resized image; it may reach past the image, where ``fill`` shows.  canvas:
    (h, w) the crop is placed on at the top left, default the crop's size; canvas outside the crop is ``fill``.
    flip_in mirrors the source before the resize (the COCO LSJ order: RandomFlip, ResizeScale, FixedSizeCrop);
    flip_out mirrors the crop window after it (the TTA, semantic and video order: resize, crop, flip).  fill: the
    byte of canvas pixels outside crop and image (128 for LSJ images); label_views uses its ``seg_pad`` instead.
    color: a :class:`bm2f_amd.color_aug.ColorAug` applied to the pixels that show the image, after resize, crop and
    flip (the mappers' order) and before the normalisation; label_views ignores it.
    """
    size: tuple
    source: int = 0
    crop: tuple | None = None
    canvas: tuple | None = None
    flip_in: bool = False
    flip_out: bool = False
    fill: int = 0
    color: _ca.ColorAug | None = None


# ------------------------------------------------------------------------------------------------ host tables
@functools.lru_cache(maxsize=512)
def bilinear_table(n_in, n_out):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the triangle filter: ``(bounds (n_out, 2) int32 =
    (xmin, n), coeffs (n_out, ksize) int32)``, or None when the axis keeps its size (PIL then skips the pass)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"axis sizes {(n_in, n_out)} must be positive")
    if n_in == n_out:
        return None
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs                                    # the triangle filter's support is 1.0
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # C's (int): truncation
    n = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < n[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for k in range(ksize):                          # C sums in this order
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    w = np.where(x < n[:, None], w, 0.0)
    coeffs = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS)).astype(np.int64)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    coeffs = coeffs.astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=512)
def nearest_table(n_in, n_out):
    """``ImagingScaleAffine``'s source index per output (int32): ``xo = a / 2``, then ``idx = int(xo); xo += a`` as a
    running fp64 sum, which is not ``(x + 0.5) * a``."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"axis sizes {(n_in, n_out)} must be positive")
    a = n_in / n_out
    steps = np.full(n_out, a, dtype=np.float64)
    steps[0] = a * 0.5
    idx = np.minimum(np.add.accumulate(steps).astype(np.int64), n_in - 1).astype(np.int32)
    idx.setflags(write=False)
    return idx


def _ksize(n_in, n_out):
    return 0 if n_in == n_out else 2 * int(math.ceil(max(n_in / n_out, 1.0))) + 1


# ------------------------------------------------------------------------------------------------ size helpers
def resize_shortest_edge_size(h, w, size, max_size):
    """``ResizeShortestEdge.get_transform``'s output size (augmentation.py:60-72): the short side becomes ``size``,
    the long side ``size / short * long``; if the larger exceeds ``max_size`` both are rescaled by ``max_size /
    larger``; each is then ``int(v + 0.5)``.  Not run against detectron2 (see the module docstring)."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f"image size {(h, w)} must be positive")
    scale = size * 1.0 / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def lsj_view(h, w, image_size, scale, offset_frac, flip, source=0):
    """The large-scale-jitter view of an (h, w) image as a :class:`View`: detectron2's ``RandomFlip``,
    ``ResizeScale(min_scale, max_scale, image_size, image_size)`` and ``FixedSizeCrop((image_size, image_size))``
    (image pad 128; label_views takes ``seg_pad=255``), given their random numbers: ``scale`` is ResizeScale's
    uniform draw, ``offset_frac`` FixedSizeCrop's single uniform draw in [0, 1) and ``flip`` RandomFlip's outcome.

    ResizeScale: ``r = min(image_size * scale / h, image_size * scale / w)``, size = round-half-even of ``(h r, w
    r)``.  FixedSizeCrop: offset = round-half-even of ``max(size - image_size, 0) * offset_frac`` per axis, a window
    of ``image_size`` squared from there (cut where the image ends), padded at the bottom and right to ``image_size``
    squared.  Not run against detectron2 (see the module docstring)."""
    h, w, S = int(h), int(w), int(image_size)
    if h <= 0 or w <= 0 or S <= 0:
        raise ValueError("sizes must be positive")
    target = S * float(scale)
    r = min(target / h, target / w)
    rh, rw = int(np.round(h * r)), int(np.round(w * r))
    oy = int(np.round(max(rh - S, 0) * float(offset_frac)))
    ox = int(np.round(max(rw - S, 0) * float(offset_frac)))
    return View(size=(rh, rw), source=source, crop=(oy, ox, S, S), canvas=(S, S), flip_in=bool(flip), fill=128)


# ------------------------------------------------------------------------------------------------ the plan
def _round_up(v, d):
    return (v + d - 1) // d * d if d > 1 else v


class _Plan:
    """The table of a call: ``rows`` (V, _FIELDS) int64 without source offsets and strides (columns 0, 3, 17: filled
    per device), ``tables`` int32, the padded size and the canvases."""

    def __init__(self, views, shapes, image):
        if len(views) == 0:
            raise ValueError("the view list is empty")
        rows = np.zeros((len(views), _FIELDS), dtype=np.int64)
        parts, where, total = [], {}, 0

        def put(key, arrays):
            nonlocal total
            if key not in where:
                where[key] = total
                for a in arrays:
                    parts.append(np.ascontiguousarray(a, dtype=np.int32).reshape(-1))
                    total += parts[-1].size
            return where[key]

        self.views, self.sizes = list(views), []
        for i, v in enumerate(self.views):
            if not 0 <= int(v.source) < len(shapes):
                raise ValueError(f"view {i}: source {v.source} outside the {len(shapes)} sources")
            H, W = shapes[v.source]
            rh, rw = (int(s) for s in v.size)
            crop = (0, 0, rh, rw) if v.crop is None else tuple(int(s) for s in v.crop)
            canvas = crop[2:] if v.canvas is None else tuple(int(s) for s in v.canvas)
            if min(H, W, rh, rw, crop[2], crop[3], canvas[0], canvas[1]) <= 0:
                raise ValueError(f"view {i}: every size must be positive")
            if not 0 <= int(v.fill) <= 255 and image:
                raise ValueError(f"view {i}: fill {v.fill} is not a byte")
            kx, ky = (_ksize(W, rw), _ksize(H, rh)) if image else (0, 0)
            if max(kx, ky) > MAX_KSIZE:
                raise ValueError(f"view {i}: {(H, W)} -> {(rh, rw)} is a down-scale beyond 65x (ksize {max(kx, ky)} > "
                                 f"{MAX_KSIZE})")
            if image:
                tx = put(("b", W, rw), bilinear_table(W, rw)) if kx else 0
                ty = put(("b", H, rh), bilinear_table(H, rh)) if ky else 0
            else:
                tx, ty = put(("n", W, rw), [nearest_table(W, rw)]), put(("n", H, rh), [nearest_table(H, rh)])
            rows[i] = (0, H, W, 0, rh, rw, *crop, *canvas, int(v.flip_in), int(v.flip_out), tx, ty, int(v.fill), 0,
                       kx, ky)
            self.sizes.append(canvas)
        self.rows = rows
        # the colour table and OpenCV's two division tables, only when a view asks for them
        self.colors, self.hsv_off = None, -1
        colored = [getattr(v, "color", None) for v in self.views] if image else []
        if any(c is not None and c.ops for c in colored):
            self.colors = np.stack([_ca.encode(c) for c in colored])
            if any(c is not None and c.needs_hsv for c in colored):
                self.hsv_off = put(("hsv",), _ca.hsv_tables())
        self.tables = np.concatenate(parts) if parts else np.zeros(1, dtype=np.int32)

    def padded(self, size_divisibility):
        d = int(size_divisibility)
        return (_round_up(max(s[0] for s in self.sizes), d), _round_up(max(s[1] for s in self.sizes), d))


def _span(tensors, extents):
    """The sources, left where they are, as one address range: (base pointer, elements, element offset per source)."""
    size = tensors[0].element_size()
    base = min(t.data_ptr() for t in tensors)
    if any((t.data_ptr() - base) % size for t in tensors):
        raise ValueError("the sources are not aligned to their element size")
    end = max(t.data_ptr() + e * size for t, e in zip(tensors, extents))
    return base, (end - base) // size, [(t.data_ptr() - base) // size for t in tensors]


def _upload_plan(plan, dev):
    """The view table, the colour table (when there is one) and the axis tables in one buffer, one copy: -> (device
    buffer, rows pointer, tables pointer, colours pointer or None)."""
    V = plan.rows.shape[0]
    nc = 0 if getattr(plan, "colors", None) is None else V * _ca.FIELDS * 2
    buf = np.empty(V * _FIELDS * 2 + nc + plan.tables.size, dtype=np.int32)
    buf[:V * _FIELDS * 2] = plan.rows.reshape(-1).view(np.int32)
    if nc:
        buf[V * _FIELDS * 2:V * _FIELDS * 2 + nc] = np.ascontiguousarray(plan.colors).reshape(-1).view(np.int32)
    buf[V * _FIELDS * 2 + nc:] = plan.tables
    d = torch.from_numpy(buf).to(dev, non_blocking=True)
    rows = d.data_ptr()
    return d, rows, rows + V * _FIELDS * 8 + nc * 4, (rows + V * _FIELDS * 8 if nc else None)


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ CPU definition
def _pass_np(img, table, axis):
    """One pass of ImagingResample on an (H, W, C) uint8 array along ``axis`` (0 vertical, 1 horizontal)."""
    if table is None:
        return img
    bounds, coeffs = table
    src = np.moveaxis(img, axis, 0).astype(np.int64)             # (n_in, ...)
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(coeffs.shape[1])[None, :], src.shape[0] - 1)
    acc = np.full((coeffs.shape[0],) + src.shape[1:], 1 << (_PRECISION_BITS - 1), dtype=np.int64)
    for k in range(coeffs.shape[1]):                             # coefficients past n are zero
        acc += src[idx[:, k]] * coeffs[:, k].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
    out = np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def _resize_bilinear_np(img, size):
    H, W = img.shape[:2]
    return _pass_np(_pass_np(img, bilinear_table(W, size[1]), 1), bilinear_table(H, size[0]), 0)


def _resize_nearest_np(planes, size):
    H, W = planes.shape[-2:]
    return planes[..., nearest_table(H, size[0]).astype(np.int64), :][..., nearest_table(W, size[1]).astype(np.int64)]


def _place_np(resized, row, fill, channels_last):
    """Crop window, flip_out and canvas of one view on a resized array ((h, w, C) or (P, h, w))."""
    if channels_last:
        resized = np.moveaxis(resized, 2, 0)
    cy0, cx0, ch, cw, Hc, Wc = (int(v) for v in row[6:12])
    rh, rw = resized.shape[-2:]
    win = np.full(resized.shape[:1] + (ch, cw), fill, dtype=resized.dtype)
    ya, yb, xa, xb = max(cy0, 0), min(cy0 + ch, rh), max(cx0, 0), min(cx0 + cw, rw)
    if yb > ya and xb > xa:
        win[:, ya - cy0:yb - cy0, xa - cx0:xb - cx0] = resized[:, ya:yb, xa:xb]
    if row[13]:
        win = win[:, :, ::-1]
    canvas = np.full(resized.shape[:1] + (Hc, Wc), fill, dtype=resized.dtype)
    canvas[:, :min(ch, Hc), :min(cw, Wc)] = win[:, :min(ch, Hc), :min(cw, Wc)]
    return canvas


def _color_np(canvas, resized_hw, row, aug):
    """The colour operations on the pixels of a (3, Hc, Wc) canvas that show the image, in place: fill stays."""
    shown = _place_np(np.ones(tuple(resized_hw) + (1,), dtype=np.uint8), row, 0, True)[0].astype(bool)
    if shown.any():
        canvas[:, shown] = _ca.apply_color(np.ascontiguousarray(canvas[:, shown].T)[None], aug)[0].T


def _norm_torch(canvas, mean, std, out_dtype):
    """uint8 (3, h, w) tensor -> the stored values: the model's (x - pixel_mean) / pixel_std in fp32."""
    if out_dtype == torch.uint8:
        return canvas
    x = canvas.float()
    if mean is not None:
        x = (x - mean.view(3, 1, 1)) / std.view(3, 1, 1)
    return x.to(out_dtype)


# ------------------------------------------------------------------------------------------------ public surface
def _mean_std(pixel_mean, pixel_std, out_dtype):
    if (pixel_mean is None) != (pixel_std is None):
        raise ValueError("pixel_mean and pixel_std come together")
    if pixel_mean is None:
        return None, None
    if out_dtype == torch.uint8:
        raise ValueError("a uint8 output stores the pixel itself: pixel_mean and pixel_std must be absent")
    mean = torch.as_tensor(pixel_mean, dtype=torch.float32).detach().cpu().reshape(-1)
    std = torch.as_tensor(pixel_std, dtype=torch.float32).detach().cpu().reshape(-1)
    if mean.numel() != 3 or std.numel() != 3 or not bool((std != 0).all()):
        raise ValueError("pixel_mean and pixel_std must hold 3 values, std nonzero")
    return mean, std


def _as_list(x):
    return [x] if isinstance(x, torch.Tensor) else list(x)


def _out_code(out_dtype):
    if out_dtype == torch.uint8:
        return _U8
    return _native.dtype_code(out_dtype, "image_views out_dtype")


def _launch_image(src_ptr, src_numel, plan, rows, out, mean, std, pad_value):
    """rows: plan.rows with the source offsets and strides filled in.  One upload, one launch."""
    dev = out.device
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    keep, rows_dev, tables_dev, colors_dev = _upload_plan(_with_rows(plan, rows), dev)
    m, s = ((0.0,) * 3, (1.0,) * 3) if mean is None else (mean.tolist(), std.tolist())
    store = (int(mean is not None), *m, *s, float(pad_value), _out_code(out.dtype), out.data_ptr(), out.shape[2],
             out.shape[3], _native.stream(dev))
    if colors_dev is None:
        _native.call("m2f_image_views", src_ptr, src_numel, _host_ptr(rows), rows_dev, rows.shape[0], tables_dev,
                     plan.tables.size, *store)
    else:
        colors = np.ascontiguousarray(plan.colors, dtype=np.float64)
        common = (src_ptr, src_numel, _host_ptr(rows), rows_dev, rows.shape[0], tables_dev, plan.tables.size,
                  _host_ptr(colors), colors_dev, int(plan.hsv_off))
        sums = None
        if bool((colors[:, 2] >= 0).any()):                  # a contrast blend: the views' sums first, device only
            sums = _native.workspace("m2f_image_views_sum_workspace", _host_ptr(rows), rows.shape[0], out.shape[2],
                                     out.shape[3], device=dev, dtype=torch.int64)
            _native.call("m2f_image_views_sum", *common, out.shape[2], out.shape[3], sums.data_ptr(), sums.numel(),
                         _native.stream(dev))
        _native.call("m2f_image_views_color", *common, _native.ptr(sums), *store)
        del sums
    del keep


def _with_rows(plan, rows):
    p = copy.copy(plan)
    p.rows = np.ascontiguousarray(rows, dtype=np.int64)
    return p


def _check_out(out, shape, dtype, dev):
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or out.device != dev
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {shape} tensor of {dtype} on {dev}")


def image_views(images, views, *, pixel_mean=None, pixel_std=None, out_dtype, size_divisibility=0, pad_value=0.0,
                out=None):
    """All ``views`` of the uint8 (H, W, 3) ``images`` (a tensor or a list; a row-strided crop view of a larger
    tensor is read in place) as one (V, 3, Hp, Wp) batch of ``out_dtype`` (uint8, float32, float16, bfloat16).

    Returns ``(batch, image_sizes)``: ``image_sizes`` the views' canvases, (Hp, Wp) their maximum rounded up to
    ``size_divisibility`` as ``ImageList.from_tensors`` does.  Inside a canvas the PIL pixel (or the view's fill) is
    stored as it is (uint8), as a float, or with ``pixel_mean`` / ``pixel_std`` as ``(float(p) - mean[c]) / std[c]``,
    bitwise torch's fp32 expression, rounded once more for a 16-bit output; outside it ``pad_value``.  On HIP tensors
    this is one upload and one launch, and every element of the batch is written (``out``, when given, is that
    batch: its contents on entry do not matter).  Raises ValueError for a source
    that is not uint8 (H, W, 3), an empty view list, mean / std with a uint8 output and a down-scale beyond 65x."""
    images = _as_list(images)
    if out_dtype not in (torch.uint8, torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"out_dtype {out_dtype} is not uint8, float32, float16 or bfloat16")
    mean, std = _mean_std(pixel_mean, pixel_std, out_dtype)
    if len(images) == 0:
        raise ValueError("no source image")
    for im in images:
        if im.dtype != torch.uint8:
            raise ValueError(f"a source image must be uint8, got {im.dtype} (float images are not resized with PIL)")
        if im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"a source image must be (H, W, 3), got {tuple(im.shape)}")
        if im.device != images[0].device:
            raise ValueError("the sources lie on different devices")
    plan = _Plan(views, [tuple(im.shape[:2]) for im in images], image=True)
    Hp, Wp = plan.padded(size_divisibility)
    dev = images[0].device
    V = len(plan.views)
    _check_out(out, (V, 3, Hp, Wp), out_dtype, dev)
    if dev.type == "cuda":
        images = [im if (im.stride(2) == 1 and im.stride(1) == 3 and im.stride(0) >= 3 * im.shape[1])
                  else im.contiguous() for im in images]
        base, numel, offs = _span(images, [(im.shape[0] - 1) * im.stride(0) + 3 * im.shape[1] for im in images])
        rows = plan.rows.copy()
        for i, v in enumerate(plan.views):
            rows[i, 0], rows[i, 3] = offs[v.source], images[v.source].stride(0)
        out = torch.empty((V, 3, Hp, Wp), dtype=out_dtype, device=dev) if out is None else out
        _launch_image(base, numel, plan, rows, out, mean, std, pad_value)
        return out, list(plan.sizes)
    pad = int(pad_value) if out_dtype == torch.uint8 else pad_value
    out = torch.empty((V, 3, Hp, Wp), dtype=out_dtype) if out is None else out
    out.fill_(pad)
    for i, v in enumerate(plan.views):
        img = images[v.source].numpy()
        r = _resize_bilinear_np(img[:, ::-1] if v.flip_in else img, plan.rows[i, 4:6])
        canvas = np.ascontiguousarray(_place_np(r, plan.rows[i], int(v.fill), True))
        if v.color is not None and v.color.ops:
            _color_np(canvas, r.shape[:2], plan.rows[i], v.color)
        canvas = torch.from_numpy(canvas)
        out[i, :, :canvas.shape[1], :canvas.shape[2]] = _norm_torch(canvas, mean, std, out_dtype)
    return out, list(plan.sizes)


def _launch_label(src_ptr, elem_bytes, src_numel, plan, rows, out):
    dev = out.device
    keep, rows_dev, tables_dev, _ = _upload_plan(_with_rows(plan, rows), dev)
    _native.call("m2f_label_views", src_ptr, elem_bytes, src_numel, _host_ptr(rows), rows_dev, rows.shape[0],
                 out.shape[1], tables_dev, plan.tables.size, out.data_ptr(), out.shape[2], out.shape[3],
                 _native.stream(dev))
    del keep


def label_views(planes, views, *, seg_pad, size_divisibility=0, out=None):
    """All ``views`` of label planes, resized with PIL's ``NEAREST``: ``planes`` is a (P, H, W) tensor or a list of
    them (uint8, int16 or int32; a label map is P = 1, instance masks P = G; one P and dtype per call; a 2-D
    tensor counts as P = 1).  Returns ``((V, P, Hp, Wp) batch of the same dtype, image_sizes)``.  ``seg_pad`` (255
    for label maps, 0 for masks) fills the canvas outside crop and image and the batch pad beyond it; the views'
    geometry is that of :func:`image_views` (``View.fill`` is not used)."""
    planes = [p[None] if p.dim() == 2 else p for p in _as_list(planes)]
    if len(planes) == 0:
        raise ValueError("no source planes")
    p0 = planes[0]
    for p in planes:
        if p.dtype not in LABEL_DTYPES:
            raise ValueError(f"label planes must be uint8, int16 or int32, got {p.dtype}")
        if p.dim() != 3 or p.shape[0] != p0.shape[0] or p.dtype != p0.dtype or p.device != p0.device:
            raise ValueError("the sources must be (P, H, W) with one P, dtype and device")
    if p0.shape[0] <= 0:
        raise ValueError("no planes")
    _, lo, hi = LABEL_DTYPES[p0.dtype]
    if not lo <= int(seg_pad) <= hi:
        raise ValueError(f"seg_pad {seg_pad} does not fit {p0.dtype}")
    views = [dataclasses.replace(v, fill=0, color=None) for v in views]
    plan = _Plan(views, [tuple(p.shape[1:]) for p in planes], image=False)
    plan.rows[:, 16] = int(seg_pad)
    Hp, Wp = plan.padded(size_divisibility)
    V, P, dev = len(plan.views), p0.shape[0], p0.device
    _check_out(out, (V, P, Hp, Wp), p0.dtype, dev)
    if dev.type == "cuda":
        planes = [p if (p.stride(2) == 1 and p.stride(1) >= p.shape[2] and p.stride(0) >= 0) else p.contiguous()
                  for p in planes]
        base, numel, offs = _span(planes, [(P - 1) * p.stride(0) + (p.shape[1] - 1) * p.stride(1) + p.shape[2]
                                           for p in planes])
        rows = plan.rows.copy()
        for i, v in enumerate(plan.views):
            s = planes[v.source]
            rows[i, 0], rows[i, 3], rows[i, 17] = offs[v.source], s.stride(1), s.stride(0)
        out = torch.empty((V, P, Hp, Wp), dtype=p0.dtype, device=dev) if out is None else out
        _launch_label(base, p0.element_size(), numel, plan, rows, out)
        return out, list(plan.sizes)
    out = torch.empty((V, P, Hp, Wp), dtype=p0.dtype) if out is None else out
    out.fill_(int(seg_pad))
    for i, v in enumerate(plan.views):
        src = planes[v.source].numpy()
        r = _resize_nearest_np(src[:, :, ::-1] if v.flip_in else src, plan.rows[i, 4:6])
        canvas = torch.from_numpy(np.ascontiguousarray(_place_np(r, plan.rows[i], int(seg_pad), False)))
        out[i, :, :canvas.shape[1], :canvas.shape[2]] = canvas
    return out, list(plan.sizes)


def resize_image(img, size):
    """``Image.fromarray(img).resize((w, h), BILINEAR)`` of a uint8 (H, W, 3) tensor as a (3, h, w) uint8 tensor."""
    return image_views([img], [View(size=tuple(int(s) for s in size))], out_dtype=torch.uint8)[0][0]


def _hwc(image, device):
    """A mapper's (3, H, W) uint8 "image" as a contiguous (H, W, 3) tensor on ``device``: one upload at most."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"\"image\" must be (3, H, W), got {tuple(image.shape)}")
    if image.dtype != torch.uint8:
        raise ValueError(f"\"image\" must be uint8, got {image.dtype} (float images are not resized with PIL)")
    if device is None or image.device == torch.device(device):
        return image.permute(1, 2, 0).contiguous()
    return image.permute(1, 2, 0).contiguous().to(device, non_blocking=True)


def preprocess_test_images(batched_inputs, *, min_size, max_size, pixel_mean, pixel_std, size_divisibility,
                           out_dtype=torch.float32, device=None):
    """The eval path from decoded images to the model's input batch: the eval mapper's ``ResizeShortestEdge(min_size,
    max_size)`` and the model's normalise, pad and stack, one launch for the batch.  ``batched_inputs``: dicts with
    a uint8 (3, H, W) ``"image"``, all on one device (moved to ``device`` when given).  Returns ``(batch (B, 3, Hp,
    Wp), image_sizes)``."""
    images = [_hwc(x["image"], device) for x in batched_inputs]
    views = [View(size=resize_shortest_edge_size(*im.shape[:2], min_size, max_size), source=i)
             for i, im in enumerate(images)]
    return image_views(images, views, pixel_mean=pixel_mean, pixel_std=pixel_std, out_dtype=out_dtype,
                       size_divisibility=size_divisibility)


class DeviceTTAMapper:
    """``DatasetMapperTTA`` for :class:`SemanticSegmentorWithTTA` (``tta_mapper=``) with PIL's exact pixels: per entry
    of ``min_sizes`` a ``ResizeShortestEdge(size, max_size)`` view of the uint8 (3, H, W) ``"image"`` and, with
    ``flip``, the same view mirrored after the resize.  One upload of the image (none when it is on ``device``
    already) and one launch give all V uint8 (3, h, w) views; they are slices of one (V, 3, Hp, Wp) batch.  The views
    are sized from the image's own shape, as detectron2's mapper does.  Returns copies of the input dict with
    ``"image"`` and ``"flipped"``."""

    def __init__(self, min_sizes, max_size, flip=True, device=None):
        self.min_sizes = tuple(int(s) for s in min_sizes)
        self.max_size = int(max_size)
        self.flip = bool(flip)
        self.device = device
        if not self.min_sizes:
            raise ValueError("min_sizes is empty")

    def __call__(self, x):
        img = _hwc(x["image"], self.device)
        sizes = tta_view_sizes(*img.shape[:2], self.min_sizes, self.max_size, self.flip)
        batch, _ = image_views([img], [View(size=(h, w), flip_out=f) for h, w, f in sizes], out_dtype=torch.uint8)
        views = []
        for i, (h, w, f) in enumerate(sizes):
            view = copy.copy(x)
            view["image"] = batch[i, :, :h, :w]
            view["flipped"] = f
            views.append(view)
        return views
