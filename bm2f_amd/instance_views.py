"""Instance masks under the input views: from source-size bit planes to per-view masks, tight boxes and areas.

The reference's instance mappers (``COCOInstanceNewBaselineDatasetMapper``, ``MaskFormerInstanceDatasetMapper``,
``YTVISDatasetMapper``) decode every annotation to a uint8 mask, push it through the image's transforms
(``transform_instance_annotations``: PIL ``NEAREST`` resize, crop, flip, zero pad) and take
``BitMasks.get_bounding_boxes`` of the result.  :func:`instance_views` is that step for a whole batch, a ragged
number of instances per image, on the packed bit planes of ``rle_to_bits_ragged`` / ``polygons_to_bits_ragged``:

  * the views are the :class:`~bm2f_amd.image_views.View` rows of ``label_views`` (the same ``_Plan`` and the same
    ``nearest_table``), so the geometry is defined once;
  * output pixel ``(y, x)`` of mask ``m`` under its view is 0 for ``y >= Hc`` or ``x >= Wc``; otherwise, with ``ry =
    cy0 + y`` and ``rx = cx0 + (flip_out ? cw - 1 - x : x)``, the source bit ``(taby[ry], flip_in ? W - 1 - tabx[rx] :
    tabx[rx])`` when ``y < ch``, ``x < cw``, ``0 <= ry < rh`` and ``0 <= rx < rw``, else 0.  Set tail bits of the source
    and the words between its planes are ignored;
  * the box of an output mask is ``[first x, first y, last x + 1, last y + 1]`` of its set pixels, zeros when there is
    none; the area is their number.

On a HIP tensor ``m2f_bits_views`` (``csrc/bits_views.hip``) does this in two launches from one uploaded table, with
no device-to-host copy.  On CPU tensors the same definition runs in numpy; that is the definition, not a fallback: on
a HIP tensor a kernel error raises ``NativeError``.

Oracle: tests/test_instance_views_cpu.py runs the definition against Pillow live, and tests/golden/instance_views.npz
records Pillow's outputs for machines without it.  detectron2 is not installed where this was written and was never
run against it.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native
from .image_views import _FIELDS, View, _host_ptr, _Plan
from .mask_iou import MAX_RAGGED_WORDS, _check_size, _pack_rows

_MASK_FIELDS = 4                        # include/bm2f.h: M2F_BITS_VIEW_MASK_FIELDS
_FORMS = {"bits": 0, "uint8": 1}        # M2F_BITS_VIEW_BITS, M2F_BITS_VIEW_BYTES


def _check_words(words):
    if not torch.is_tensor(words) or words.dim() != 1 or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("words must be a flat contiguous int32 tensor")
    if words.numel() > MAX_RAGGED_WORDS:
        raise ValueError(f"words holds {words.numel()} words, more than the {MAX_RAGGED_WORDS} of one call")


def _mask_table(words, offsets, sizes, view_of_mask, views):
    """Every check of the per-mask table -> (M, 4) int64 rows (word offset, H, W, view)."""
    try:
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        vom = np.asarray(view_of_mask, dtype=np.int64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError("offsets and view_of_mask must be (M,) and sizes (M, 2) integers") from e
    M = offsets.size
    if hw.shape[0] != M or vom.size != M:
        raise ValueError(f"{hw.shape[0]} sizes and {vom.size} view indices for {M} offsets")
    for m in range(M):
        _check_size(int(hw[m, 0]), int(hw[m, 1]), f"mask {m}: ")
    if M and (vom.min() < 0 or vom.max() >= len(views)):
        raise ValueError(f"a view index is outside the {len(views)} views")
    fw = hw[:, 0] * ((hw[:, 1] + 31) // 32)
    if M and (offsets.min() < 0 or (offsets + fw).max() > words.numel()):
        raise ValueError(f"a plane does not fit the buffer of {words.numel()} words")
    return np.ascontiguousarray(np.concatenate((offsets[:, None], hw, vom[:, None]), axis=1))


def _plan(views, masks):
    """The views as a ``label_views`` plan whose source ``i`` is view ``i``'s own (H, W): the size of its masks."""
    V = len(views)
    shapes = [None] * V
    for m in range(masks.shape[0]):
        v, hw = int(masks[m, 3]), (int(masks[m, 1]), int(masks[m, 2]))
        if shapes[v] is not None and shapes[v] != hw:
            raise ValueError(f"mask {m} is {hw}, another mask of view {v} is {shapes[v]}: one source size per view")
        shapes[v] = hw
    rows = [dataclasses.replace(v, source=i, fill=0, color=None) for i, v in enumerate(views)]
    # a view without masks draws nothing: any source size serves its row
    plan = _Plan(rows, [s if s is not None else (1, 1) for s in shapes], image=False)
    plan.rows[:, 3] = plan.rows[:, 2]   # rows of W elements: what the bit kernel's row check expects (bm2f.h)
    return plan


def _unpack(plane, W):
    bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), axis=-1, bitorder="little")
    return bits[:, :W]


def _view_np(mask, row, tables):
    """The definition on one (H, W) uint8 mask: -> (Hc, Wc) uint8."""
    H, W, rh, rw, cy0, cx0, ch, cw, Hc, Wc, flip_in, flip_out, tx, ty = (int(v) for v in row[1:3].tolist()
                                                                         + row[4:16].tolist())
    taby, tabx = tables[ty:ty + rh].astype(np.int64), tables[tx:tx + rw].astype(np.int64)
    y, x = np.arange(Hc, dtype=np.int64), np.arange(Wc, dtype=np.int64)
    ry, rx = cy0 + y, cx0 + (cw - 1 - x if flip_out else x)
    oky, okx = (y < ch) & (ry >= 0) & (ry < rh), (x < cw) & (rx >= 0) & (rx < rw)
    sy, sx = taby[np.clip(ry, 0, rh - 1)], tabx[np.clip(rx, 0, rw - 1)]
    if flip_in:
        sx = W - 1 - sx
    return np.where(oky[:, None] & okx[None, :], mask[sy][:, sx], 0).astype(np.uint8)


def _stats_np(mask):
    """x0, y0, x1, y1, area of a 2-D mask: ``BitMasks.get_bounding_boxes`` and the pixel count."""
    xs, ys = np.flatnonzero(mask.any(axis=0)), np.flatnonzero(mask.any(axis=1))
    if xs.size == 0:
        return (0, 0, 0, 0, 0)
    return (int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1, int(np.count_nonzero(mask)))


def instance_views(words, offsets, sizes, view_of_mask, views, *, size_divisibility=0, out="bits", into=None):
    """The masks of a batch under their views.  ``words``: the flat int32 bit planes of ``rle_to_bits_ragged`` /
    ``polygons_to_bits_ragged``, mask ``m`` of ``sizes[m] = (H, W)`` at the word offset ``offsets[m]``;
    ``view_of_mask[m]`` indexes ``views``, a list of :class:`~bm2f_amd.image_views.View` (``View.source``, ``fill``
    and ``color`` are not used: a view's source is the masks that name it, which must share one size).

    Returns ``(masks, boxes, areas, image_sizes)``: ``masks`` (M, Hp, ceil(Wp / 32)) int32 bit planes with zero tail
    bits (``out="bits"``) or (M, Hp, Wp) uint8 of 0 / 1 (``out="uint8"``), zero outside canvas, crop and image;
    ``boxes`` (M, 4) float32 ``x0, y0, x1, y1`` of the output mask, zeros for an empty one; ``areas`` (M,) int32;
    ``image_sizes`` the views' canvases, (Hp, Wp) their maximum rounded up to ``size_divisibility``.  On a HIP tensor:
    one table upload, the two launches of ``m2f_bits_views`` and no device-to-host copy, whatever the numbers of
    images and instances.  ``into``, when given, is the ``masks`` tensor to fill: every word or byte of it is
    written, so its contents on entry do not matter.

    Raises ValueError, before any launch, for a ``words`` that is not a flat contiguous int32 tensor of at most
    ``MAX_RAGGED_WORDS`` words, an empty view list, a size that is not positive or has ``H W >= 2^31``, a plane
    outside the buffer, a view index out of range, two source sizes under one view and an output beyond
    ``MAX_RAGGED_WORDS`` words."""
    if out not in _FORMS:
        raise ValueError(f"out {out!r} is not \"bits\" or \"uint8\"")
    _check_words(words)
    views = list(views)
    if not views:
        raise ValueError("the view list is empty")
    masks = _mask_table(words, offsets, sizes, view_of_mask, views)
    plan = _plan(views, masks)
    Hp, Wp = plan.padded(size_divisibility)
    _check_size(Hp, Wp, "the output plane: ")
    M, wordsp, dev = masks.shape[0], (Wp + 31) // 32, words.device
    out_words = M * (Hp * wordsp if out == "bits" else (Hp * Wp + 3) // 4)
    if out_words > MAX_RAGGED_WORDS:
        raise ValueError(f"the output takes {out_words} words, more than the {MAX_RAGGED_WORDS} of one call")
    shape = (M, Hp, wordsp) if out == "bits" else (M, Hp, Wp)
    dtype = torch.int32 if out == "bits" else torch.uint8
    if into is not None and (tuple(into.shape) != shape or into.dtype != dtype or into.device != dev
                             or not into.is_contiguous()):
        raise ValueError(f"into must be a contiguous {shape} tensor of {dtype} on {dev}")
    if M == 0:
        return (torch.zeros(shape, dtype=dtype, device=dev), torch.zeros((0, 4), dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev), list(plan.sizes))
    if dev.type == "cuda":
        V = plan.rows.shape[0]
        buf = np.concatenate((plan.rows.reshape(-1).view(np.int32), masks.reshape(-1).view(np.int32), plan.tables))
        d = torch.from_numpy(buf).to(dev, non_blocking=True)                      # one copy
        rows_dev = d.data_ptr()
        masks_dev = rows_dev + V * _FIELDS * 8
        res = torch.empty(shape, dtype=dtype, device=dev) if into is None else into
        stats = torch.empty((M, 5), dtype=torch.int32, device=dev)
        ws = _native.workspace("m2f_bits_views_workspace", M, Hp, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            _native.call("m2f_bits_views", words.data_ptr(), words.numel(), _host_ptr(plan.rows), rows_dev, V,
                         masks_dev + M * _MASK_FIELDS * 8, plan.tables.size, _host_ptr(masks), masks_dev, M,
                         _FORMS[out], res.data_ptr(), Hp, Wp, stats.data_ptr(), ws.data_ptr(), ws.numel(),
                         _native.stream(dev))
        del d, ws
        return res, stats[:, :4].float(), stats[:, 4], list(plan.sizes)
    src = words.detach().numpy()
    dense = np.zeros((M, Hp, Wp), dtype=np.uint8)
    stats = np.zeros((M, 5), dtype=np.int32)
    for m, (off, H, W, v) in enumerate(masks.tolist()):
        wr = (W + 31) // 32
        plane = _unpack(src[off:off + H * wr].reshape(H, wr), W)
        o = _view_np(plane, plan.rows[v], plan.tables)
        dense[m, :o.shape[0], :o.shape[1]] = o
        stats[m] = _stats_np(dense[m])
    res = torch.from_numpy(_pack_rows(dense.astype(bool)) if out == "bits" else dense)
    if into is not None:
        res = into.copy_(res)
    stats = torch.from_numpy(stats)
    return res, stats[:, :4].float(), stats[:, 4].clone(), list(plan.sizes)


def bit_boxes_ragged(words, offsets, sizes, *, out="bits"):
    """:func:`instance_views` with identity views, for planes that are at the output size already (polygons
    rasterised on the canvas): ``(masks, boxes, areas)`` with ``masks`` (M, max H, max W [/ 32]) the planes gathered
    into one tensor, tail bits zero, and the tight boxes and areas of each.  The same kernel, the same two launches."""
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if hw.shape[0] == 0:
        raise ValueError("no planes")
    uniq, view_of = np.unique(hw, axis=0, return_inverse=True)
    views = [View(size=(int(h), int(w))) for h, w in uniq]
    masks, boxes, areas, _ = instance_views(words, offsets, hw, view_of.reshape(-1), views, out=out)
    return masks, boxes, areas
