"""Mask boundaries on one-bit-per-pixel planes: what the reference's ``tools/evaluate_coco_boundary_ap.py`` gets from
``boundary_iou.utils.boundary_utils.mask_to_boundary`` (OpenCV's ``cv2.erode`` on every detection and ground truth),
restated without either package.  Neither ``boundary_iou`` nor ``cv2`` has been run against this code; what is tested
is the definition below, the published one.

  * Dilation.  For an ``H x W`` image ``d = max(1, int(round(dilation_ratio * sqrt(H * H + W * W))))`` in float64 with
    Python's ``round``; the default ``dilation_ratio`` is 0.02.
  * Erosion.  ``cv2.erode`` with a 3 x 3 kernel of ones, ``d`` iterations, on the mask padded by one ring of zeros:
    pixel ``(y, x)`` survives exactly when every pixel of the ``(2d + 1) x (2d + 1)`` window centred on it lies inside
    the image and is set.  Everything outside the image counts as zero.
  * Boundary.  ``boundary = mask & ~erode(mask)``.
  * Boundary IoU of a detection and a ground truth is ``min(mask IoU, IoU of the two boundaries)``, both with COCO's
    crowd rule (with a crowd ground truth the union is the detection's area: of its mask, or of its boundary).

:func:`boundary_dilation`      ``d`` of an image size.
:func:`boundary_bits_ragged`   planes of any sizes in one flat word buffer (the layout of ``rle_to_bits_ragged``) ->
                               their boundary planes at the same offsets: one launch of ``m2f_bits_boundary_ragged``
                               (``csrc/mask_boundary.hip``) whatever the number of planes, dealt to workgroups by a
                               host-built table.
:func:`mask_to_boundary_bits`  the same for uniform ``(..., H, words)`` planes (``rle_to_bits``, ``pack_mask_bits``,
                               the video head's ``keep_bits=True`` output), through the same kernel.
:func:`boundary_pair_counts_ragged`
                               the Boundary AP evaluator's batch step: decode (and rasterise polygons), boundary, pair
                               counts of the masks and of the boundaries; one upload and one device-to-host copy.

On CPU tensors a numpy restatement of the same definition runs; that is not a fallback: on a HIP tensor a kernel
error raises ``NativeError``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native
from .mask_iou import (MAX_RAGGED_WORDS, _check_size, _decode_plan, _groups_by_offset, _launch_decode, _launch_pairs,
                       _pack_rows, _pair_counts_ragged_host, _pair_plan, _split_counts, rle_to_bits_ragged)
from .polygon import _crossings_host, _decode_host, _launch_polygons, _plan, _tables, is_polygon


def boundary_tiles():
    """(band_rows, tile_words, d_max) of ``m2f_bits_boundary_ragged``: the rows and words of a plane one workgroup
    owns, and the largest dilation the kernel takes."""
    return _native.query("m2f_bits_boundary_tiles", outs="iii")


def boundary_dilation(H, W, dilation_ratio=0.02) -> int:
    """``max(1, int(round(dilation_ratio * sqrt(H^2 + W^2))))``, as ``mask_to_boundary`` computes it."""
    H, W = int(H), int(W)
    return max(1, int(round(float(dilation_ratio) * math.sqrt(H * H + W * W))))


# -------------------------------------------------------------------------------------------------------------------
# checks and the table (host)
# -------------------------------------------------------------------------------------------------------------------
def _dilations(hw, dilation_ratio, dilations):
    """-> (M,) int64 ``d`` per plane, checked against [1, d_max]."""
    M = hw.shape[0]
    if dilations is None:
        d = np.array([boundary_dilation(h, w, dilation_ratio) for h, w in hw], dtype=np.int64).reshape(M)
    else:
        raw = np.asarray(dilations)
        if raw.dtype.kind not in "iu":
            raise ValueError("dilations must be integers")
        if raw.ndim == 0:
            raw = np.broadcast_to(raw, (M,))
        if raw.shape != (M,):
            raise ValueError(f"dilations of shape {raw.shape} for {M} planes")
        d = raw.astype(np.int64)
    d_max = boundary_tiles()[2]
    if d.size and (d.min() < 1 or d.max() > d_max):
        raise ValueError(f"a dilation of {int(d.min() if d.min() < 1 else d.max())} pixels is outside [1, {d_max}]")
    return d


def _boundary_plan(hw, offsets, d, total_words):
    """Every check of the planes' geometry -> (the tables of ``m2f_bits_boundary_ragged``, number of table rows)."""
    M = hw.shape[0]
    for H, W in hw:
        _check_size(int(H), int(W))
    fw = hw[:, 0] * ((hw[:, 1] + 31) // 32)
    if M and (offsets.min() < 0 or (offsets + fw).max() > total_words):
        raise ValueError(f"a plane does not fit the buffer of {total_words} words")
    band, tile_w, _ = boundary_tiles()
    col_tiles = ((hw[:, 1] + 31) // 32 + tile_w - 1) // tile_w
    ntile = (hw[:, 0] + band - 1) // band * col_tiles
    plane_of = np.repeat(np.arange(M, dtype=np.int64), ntile)
    first = np.concatenate(([0], np.cumsum(ntile)))[:-1]
    blocks = np.stack((plane_of, np.arange(plane_of.size) - first[plane_of]), axis=1).astype(np.int32)
    tables = {"bd_offsets": np.ascontiguousarray(offsets, dtype=np.int64), "bd_sizes": hw.astype(np.int32),
              "bd_dilations": d.astype(np.int32), "bd_blocks": blocks}
    return tables, blocks.shape[0]


def _launch_boundary(words, out, dev_tables, num_planes, num_blocks, max_dilation, device):
    t = dev_tables
    with torch.cuda.device(device):
        _native.call("m2f_bits_boundary_ragged", words.data_ptr(), words.numel(), num_planes, t["bd_sizes"].data_ptr(),
                     t["bd_offsets"].data_ptr(), t["bd_dilations"].data_ptr(), _native.ptr_or_null(t["bd_blocks"]),
                     num_blocks, max_dilation, out.data_ptr(), _native.stream(device))


# -------------------------------------------------------------------------------------------------------------------
# the definition in numpy
# -------------------------------------------------------------------------------------------------------------------
def _erode_dense(mask, d):
    """(H, W) bool -> the pixels whose (2d + 1)^2 window lies inside the image and is all set, by window sums of an
    integral image."""
    H, W = mask.shape
    n = 2 * d + 1
    out = np.zeros((H, W), dtype=bool)
    if H < n or W < n:
        return out
    s = np.zeros((H + 1, W + 1), dtype=np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(mask, axis=0, dtype=np.int64), axis=1)
    win = s[n:, n:] - s[:-n, n:] - s[n:, :-n] + s[:-n, :-n]           # (H - 2d, W - 2d): windows centred at (y, x) + d
    out[d:H - d, d:W - d] = win == n * n
    return out


def _unpack_rows(plane, W):
    """(H, words) int32 -> (H, W) bool; bits x >= W are dropped."""
    bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), axis=-1, bitorder="little")
    return bits[:, :W].astype(bool)


def _boundary_host(words, hw, offsets, d):
    out = np.zeros_like(words)
    for m, (H, W) in enumerate(hw):
        wr = (W + 31) // 32
        n = H * wr
        mask = _unpack_rows(words[offsets[m]:offsets[m] + n].reshape(H, wr), int(W))
        out[offsets[m]:offsets[m] + n] = _pack_rows(mask & ~_erode_dense(mask, int(d[m]))).reshape(-1)
    return out


# -------------------------------------------------------------------------------------------------------------------
# public
# -------------------------------------------------------------------------------------------------------------------
def boundary_bits_ragged(words, offsets, sizes, dilation_ratio=0.02, dilations=None) -> torch.Tensor:
    """words: a flat int32 tensor of bit planes, plane ``m`` of ``sizes[m] = (H, W)`` pixels at the word offset
    ``offsets[m]`` (what :func:`~bm2f_amd.mask_iou.rle_to_bits_ragged` and ``polygons_to_bits_ragged`` return; any
    offsets are accepted).  -> a flat int32 tensor of the same length on the same device holding the boundary planes
    at the same offsets, tail bits (``x >= W``) zero.  ``d`` is :func:`boundary_dilation` of each plane's size, or
    ``dilations`` (one integer for all or one per plane) where given.  Set tail bits of the input and the words
    between its planes are ignored; the words between the output's planes are unspecified on the device (zero on the
    CPU).  ``d >= H`` or ``d >= W`` is allowed: the erosion is empty and the boundary is the mask.  On a HIP tensor
    one upload of the table and one launch of ``m2f_bits_boundary_ragged`` whatever the number of planes and sizes.

    Raises ValueError, before any launch, when ``words`` is not a flat contiguous int32 tensor of at most
    ``MAX_RAGGED_WORDS`` words, a size is not positive, a plane does not lie inside ``words``, ``dilations`` is not
    integer or a dilation is outside ``[1, d_max]`` (``boundary_tiles()[2]``)."""
    if not torch.is_tensor(words) or words.dim() != 1 or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("words must be a flat contiguous int32 tensor")
    if words.numel() > MAX_RAGGED_WORDS:
        raise ValueError(f"words holds {words.numel()} words, more than the {MAX_RAGGED_WORDS} of one call")
    try:
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1, 2))
    except (TypeError, ValueError) as e:
        raise ValueError("offsets must be (M,) and sizes (M, 2) integers") from e
    if hw.shape[0] != offsets.size:
        raise ValueError(f"{hw.shape[0]} sizes for {offsets.size} offsets")
    if offsets.size == 0:
        return torch.zeros_like(words)
    for H, W in hw:
        _check_size(int(H), int(W))
    d = _dilations(hw, dilation_ratio, dilations)
    tables, num_blocks = _boundary_plan(hw, offsets, d, words.numel())
    if words.device.type != "cuda":
        return torch.from_numpy(_boundary_host(words.detach().numpy(), hw, offsets, d)).to(words.device)
    dev = _native.upload_tables(tables, words.device)                 # one copy
    out = torch.empty_like(words)
    _launch_boundary(words.detach(), out, dev, offsets.size, num_blocks, int(d.max()), words.device)
    return out


def mask_to_boundary_bits(planes, width, dilation_ratio=0.02, dilation=None) -> torch.Tensor:
    """planes: ``(..., H, words)`` int32 bit planes of ``width`` columns (``words = ceil(width / 32)``; set tail bits
    are ignored) -> their boundary planes, same shape and device, tail bits zero.  ``d`` is
    :func:`boundary_dilation` of ``(H, width)`` or the integer ``dilation``.  Built on the ragged kernel: one launch
    whatever the number of planes."""
    if not torch.is_tensor(planes) or planes.dim() < 2 or planes.dtype != torch.int32:
        raise ValueError("planes must be a (..., H, words) int32 tensor")
    H, wr = int(planes.shape[-2]), int(planes.shape[-1])
    W = int(width)
    if W <= 0 or H <= 0 or wr != (W + 31) // 32:
        raise ValueError("planes must be (..., H, ceil(width / 32)) with positive H and width")
    M = planes.numel() // (H * wr)
    if M == 0:
        return torch.zeros_like(planes)
    flat = planes.detach().contiguous().view(-1)
    offsets = np.arange(M, dtype=np.int64) * (H * wr)
    sizes = np.broadcast_to(np.array([H, W], dtype=np.int64), (M, 2))
    dil = None if dilation is None else np.asarray(dilation)
    return boundary_bits_ragged(flat, offsets, sizes, dilation_ratio, dil).view(planes.shape)


# -------------------------------------------------------------------------------------------------------------------
# the evaluator's batch step
# -------------------------------------------------------------------------------------------------------------------
def boundary_pair_counts_ragged(masks, groups, device=None, sizes=None, names=None, dilation_ratio=0.02):
    """:func:`~bm2f_amd.polygon.pair_counts_ragged` with the boundaries counted as well.  ``masks`` holds RLE dicts,
    ``None`` or polygon annotations (whose (H, W) ``sizes[m]`` gives); ``groups`` holds ``(H, W, a_masks, b_masks)``
    with indices into ``masks``.  -> ``(mask_counts, boundary_counts)``, each one ``(inter (na, nb), area_a (na,),
    area_b (nb,))`` of host int64 arrays per group; ``d`` is :func:`boundary_dilation` of each mask's size.

    On a HIP device: one upload, a number of launches that does not depend on the batch (the RLE decoder; with
    polygons the crossings kernel, one sort and the polygon decoder; the boundary kernel; the pair counts on the mask
    planes and on the boundary planes) and one device-to-host copy.  The boundary planes take a second buffer as large
    as the first: callers that size batches by bytes count both."""
    device = torch.device("cpu" if device is None else device)
    masks, groups = list(masks), list(groups)
    if not groups:
        return [], []
    if not masks:
        empty = [(np.zeros((0, 0), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in groups]
        return empty, list(empty)
    poly = np.array([is_polygon(m) for m in masks], dtype=bool)
    rles = [None if p else m for m, p in zip(masks, poly)]
    hw, out_offsets, total, dtables = _decode_plan(rles, sizes)
    which = np.flatnonzero(poly)
    plan = None
    if which.size:
        dtables["blocks"] = dtables["blocks"][~poly[dtables["blocks"][:, 0]]]   # the RLE decoder skips polygon planes
        plan = _plan([masks[i] for i in which], hw[which], None if names is None else [names[i] for i in which])
    desc, ptables, num_tiles = _pair_plan(_groups_by_offset(groups, hw, out_offsets), total)
    d = _dilations(hw, dilation_ratio, None)
    btables, num_blocks = _boundary_plan(hw, out_offsets, d, total)
    if device.type != "cuda":
        words = rle_to_bits_ragged(rles, device, sizes)[0].numpy()    # zero planes where the polygons go
        if plan is not None:
            words = words | _decode_host(_crossings_host(plan), plan, out_offsets[which], total)
        edges = _boundary_host(words, hw, out_offsets, d)
        return _pair_counts_ragged_host(words, desc, ptables), _pair_counts_ragged_host(edges, desc, ptables)
    poly_tables = _tables(plan, out_offsets[which]) if plan is not None else {}
    dev = _native.upload_tables({**dtables, **poly_tables, **ptables, **btables}, device)  # one copy
    words = torch.empty(total, dtype=torch.int32, device=device)
    edges = torch.empty(total, dtype=torch.int32, device=device)
    _launch_decode(dev, len(rles), words, device)
    if plan is not None:
        _launch_polygons(dev, plan, words, device)
    _launch_boundary(words, edges, dev, len(masks), num_blocks, int(d.max()), device)
    out_m = _launch_pairs(words, desc, dev, num_tiles, device)
    out_b = _launch_pairs(edges, desc, dev, num_tiles, device)
    host = torch.cat((out_m, out_b)).cpu().numpy()                    # the one copy
    return _split_counts(host[:out_m.numel()], desc), _split_counts(host[out_m.numel():], desc)
