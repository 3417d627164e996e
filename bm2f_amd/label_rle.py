"""COCO RLE of the segments of label maps, and its inverse: what detectron2's ``encode_json_sem_seg``, the reference's
``datasets/prepare_ade20k_ins_seg.py`` and the panoptic-to-detection conversion get from
``pycocotools.mask.encode(map == v)`` once per value, without a dense mask per segment.

:func:`label_maps_to_rle`   label planes -> per image, one ``{"label", "segmentation", "area", "bbox"}`` per segment.
:func:`rle_to_label_maps`   per image, ``(value, rle)`` in painting order -> label planes (a later segment overwrites).

The definition (CPU tensors, numpy): for each selected value ``rle_encode(plane == value)``, its pixel count and its
tight box ``[xmin, ymin, xmax - xmin + 1, ymax - ymin + 1]``; for the inverse ``rle_decode`` per segment in list order.
That is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.

The device route (``csrc/label_rle.hip``, ``m2f_label_rle_*`` and ``m2f_rle_paint_labels`` in ``include/bm2f.h``)
reads a label map column-major as a sequence of runs, sorts the runs by (image, label) with one stable ``torch.sort``
and writes every segment's transitions from its runs; the strings come from the unchanged string stage of
``csrc/rle.hip``.  Two device-to-host copies per call: the number of runs of every image (which sizes the run
buffers), then the segment headers, string offsets and encoded bytes in one buffer sized by bounds (the number of
segments and of characters is known on the device only).  The host never receives a label map or a mask.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native
from .label_planes import LABEL_DTYPES
from .mask_iou import _run_ends_chunked
from .rle import _GROUP_LIMITS, _encode_host, counts_to_string, rle_decode

_IMAGE_FIELDS, _HEADER_FIELDS, _PAINT_FIELDS = 8, 8, 6          # M2F_LABEL_RLE_*_FIELDS
_INT32 = (-2 ** 31, 2 ** 31 - 1)


# -------------------------------------------------------------------------------------------------------------------
# arguments
# -------------------------------------------------------------------------------------------------------------------
def _check_planes(planes):
    """-> the planes with unit column stride; every check that needs no data."""
    planes = list(planes)
    for k, p in enumerate(planes):
        if not torch.is_tensor(p) or p.dim() != 2:
            raise ValueError(f"plane {k} must be a (H, W) tensor")
        if p.dtype not in LABEL_DTYPES:
            raise ValueError(f"plane {k}: labels must be uint8, int16 or int32, got {p.dtype}")
        if p.dtype != planes[0].dtype:
            raise ValueError(f"planes of different dtypes in one batch: {planes[0].dtype} and {p.dtype}")
        if p.device != planes[0].device:
            raise ValueError("the planes of a batch must be on one device")
        if p.shape[0] * p.shape[1] >= 2 ** 31:
            raise ValueError(f"plane {k}: {p.shape[0]} x {p.shape[1]} pixels do not fit a 32-bit count")
    def in_place(p):                                                 # rows of unit stride that do not overlap
        return (p.stride(1) == 1 or p.shape[1] <= 1) and (p.stride(0) >= p.shape[1] or p.shape[0] <= 1)
    return [p.detach() if in_place(p) else p.detach().contiguous() for p in planes]


def _per_image(value, n, what):
    """None, a scalar or one entry per image -> a list of n."""
    if value is None or isinstance(value, (int, np.integer)):
        return [value if value is None else int(value)] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{len(value)} {what} for {n} planes")
    return [None if v is None else int(v) for v in value]


def _id_lists(ids, n):
    if ids is None:
        return None
    ids = list(ids)
    if len(ids) != n:
        raise ValueError(f"{len(ids)} id lists for {n} planes")
    return [[int(v) for v in (one.tolist() if hasattr(one, "tolist") else one)] for one in ids]


def _entry(label, rle, area, box):
    return {"label": int(label), "segmentation": rle, "area": int(area), "bbox": [int(v) for v in box]}


def _empty_entry(label, H, W):
    return _entry(label, {"size": [H, W], "counts": counts_to_string([H * W])}, 0, (0, 0, 0, 0))


# -------------------------------------------------------------------------------------------------------------------
# the definition
# -------------------------------------------------------------------------------------------------------------------
def _segments_host(plane, ignore, ids):
    H, W = plane.shape
    if H * W == 0:
        return []
    wide = plane.astype(np.int64)
    values = [int(v) for v in np.unique(wide) if v != ignore] if ids is None else ids
    if not values:
        return []
    masks = np.stack([(wide == v) & (v != ignore) for v in values])
    out = []
    for v, m, rle in zip(values, masks, _encode_host(masks)):
        ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        box = (xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1) if ys.size else (0, 0, 0, 0)
        out.append(_entry(v, rle, m.sum(), box))
    return out


# -------------------------------------------------------------------------------------------------------------------
# the device route
# -------------------------------------------------------------------------------------------------------------------
def _key(image, label):
    return (image << 32) | ((label & 0xffffffff) ^ 0x80000000)


def _string_bound(n, segments, N):
    """An upper bound of the characters of the ``segments`` masks of N pixels of one image that hold n counts in all:
    ``rle._char_bound`` summed without the counts of the single masks.  A mask of k counts takes at most
    2 k + 2 sum_j min(k, N // 2^(5j - 1)) characters, the k sum to n, and at most N // 2^(5j - 1) counts of one mask,
    so at most ``segments`` times as many of the image, reach 2^(5j - 1)."""
    return 2 * n + 2 * sum(min(n, segments * (N // lim)) for lim in _GROUP_LIMITS)


def _segments_device(planes, ignores, ids):
    """planes: HIP tensors of one dtype, each of at least one pixel -> per plane the list of entries."""
    dev = planes[0].device
    B = len(planes)
    nbytes, lo, hi = LABEL_DTYPES[planes[0].dtype]
    hw = np.array([p.shape for p in planes], dtype=np.int64)
    pixels = hw[:, 0] * hw[:, 1]
    col_base = np.concatenate(([0], np.cumsum(hw[:, 1])))
    block_base = np.concatenate(([0], np.cumsum((hw[:, 1] + 255) // 256)))
    images = np.zeros((B, _IMAGE_FIELDS), dtype=np.int64)
    for i, p in enumerate(planes):
        ign = ignores[i]
        images[i] = (p.data_ptr(), hw[i, 0], hw[i, 1], p.stride(0) if hw[i, 0] > 1 else max(p.stride(0), hw[i, 1]),
                     col_base[i], block_base[i], _key(i, ign) if ign is not None and lo <= ign <= hi else -1, 0)
    tables = {"images": images, "gather": col_base}
    if ids is not None:
        # the device sees every distinct id of the label range once, ascending; the host puts them back in order
        keys = sorted({_key(i, v) for i, one in enumerate(ids) for v in one if _INT32[0] <= v <= _INT32[1]})
        tables["seg_key"] = np.array(keys + [0], dtype=np.int64)     # never empty
        tables["num_segments"] = np.array([len(keys)], dtype=np.int64)
    t = _native.upload_tables(tables, dev)                            # the one upload
    st = _native.stream(dev)
    total_cols, num_blocks = int(col_base[-1]), int(block_base[-1])
    with torch.cuda.device(dev):
        counts = torch.empty(total_cols, dtype=torch.int32, device=dev)
        walk = (t["images"].data_ptr(), B, num_blocks, nbytes)
        _native.call("m2f_label_rle_col_counts", *walk, counts.data_ptr(), total_cols, st)
        col_start = torch.zeros(total_cols + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=col_start[1:])
        run_base = col_start[t["gather"]]                             # (B + 1): the first run of every image
        runs = np.diff(np.array(run_base.cpu().tolist(), dtype=np.int64))   # copy 1: B + 1 integers size the buffers
        R = int(runs.sum())
        if (runs < 1).any() or (runs > pixels).any():
            raise _native.NativeError(f"label_maps_to_rle: run counts {runs.tolist()} of planes of {pixels.tolist()} pixels")
        run_pos = torch.empty(R, dtype=torch.int32, device=dev)
        run_key = torch.empty(R, dtype=torch.int64, device=dev)
        _native.call("m2f_label_rle_runs", *walk, col_start.data_ptr(), total_cols, run_pos.data_ptr(),
                     run_key.data_ptr(), R, st)
        sorted_key, perm = torch.sort(run_key, stable=True)
        if ids is None:
            seg_cap = np.minimum(np.minimum(runs, pixels), hi - lo + 1)
            seg_key = torch.empty(int(seg_cap.sum()), dtype=torch.int64, device=dev)
            num_segments = torch.empty(1, dtype=torch.int64, device=dev)
        else:
            seg_cap = np.bincount(np.array(keys, dtype=np.int64) >> 32, minlength=B)
            seg_key, num_segments = t["seg_key"], t["num_segments"]
        S_cap = int(seg_cap.sum())
        spans = torch.empty((4, R), dtype=torch.int32, device=dev)   # start, end, ntrans, first
        _native.call("m2f_label_rle_spans", sorted_key.data_ptr(), perm.data_ptr(), R, run_pos.data_ptr(),
                     run_base.data_ptr(), t["images"].data_ptr(), B, None if ids is None else seg_key.data_ptr(),
                     None if ids is None else num_segments.data_ptr(), S_cap, spans[0].data_ptr(),
                     spans[1].data_ptr(), spans[2].data_ptr(), spans[3].data_ptr(), st)
        tscan = torch.cumsum(spans[2], 0, dtype=torch.int64)
        if ids is None:
            seg_rank = torch.cumsum(spans[3], 0, dtype=torch.int64)
            _native.call("m2f_label_rle_seg_keys", sorted_key.data_ptr(), spans[3].data_ptr(), seg_rank.data_ptr(),
                         R, seg_key.data_ptr(), S_cap, num_segments.data_ptr(), st)
        # a run gives at most two transitions and every segment slot one closing count; the slots beyond the
        # segments that exist are one-entry dummies (zeros), so the string stage runs on this capacity
        total = 2 * R + S_cap + 1
        cap = total + sum(_string_bound(int(2 * r + s), int(s), int(n)) for r, s, n in zip(runs, seg_cap, pixels))
        head = 8 * (1 + S_cap + 2)
        hdr_bytes = 4 * _HEADER_FIELDS * (S_cap + 1)
        out = torch.empty(head + hdr_bytes + cap, dtype=torch.uint8, device=dev)
        positions = torch.zeros(total, dtype=torch.int32, device=dev)
        seg_start = torch.empty(S_cap + 1, dtype=torch.int64, device=dev)
        _native.call("m2f_label_rle_segments", sorted_key.data_ptr(), R, spans[0].data_ptr(), spans[1].data_ptr(),
                     spans[2].data_ptr(), tscan.data_ptr(), t["images"].data_ptr(), B, seg_key.data_ptr(),
                     num_segments.data_ptr(), S_cap, positions.data_ptr(), total, seg_start.data_ptr(),
                     out.data_ptr() + head, st)
        delta = torch.empty(total, dtype=torch.int32, device=dev)
        nchar = torch.empty(total, dtype=torch.uint8, device=dev)
        _native.call("m2f_rle_deltas", positions.data_ptr(), seg_start.data_ptr(), S_cap + 1, 1, total,
                     delta.data_ptr(), nchar.data_ptr(), st)
        char_end = torch.cumsum(nchar, 0, dtype=torch.int64)
        first = seg_start + torch.arange(S_cap + 1, dtype=torch.int64, device=dev)
        ends = torch.cat([char_end.new_zeros(1), char_end])[first]   # the byte offset of every segment slot
        out[:8] = num_segments.view(torch.uint8)
        out[8:8 * (S_cap + 2)] = ends.view(torch.uint8)
        _native.call("m2f_rle_chars", delta.data_ptr(), nchar.data_ptr(), char_end.data_ptr(), total,
                     out.data_ptr() + head + hdr_bytes, cap, st)
        host = out.cpu().numpy()                                      # copy 2: headers, offsets and encoded bytes
    S = int(host[:8].view(np.int64)[0])
    offsets = host[8:8 * (S_cap + 2)].view(np.int64)
    headers = host[head:head + hdr_bytes].view(np.int32).reshape(S_cap + 1, _HEADER_FIELDS)
    if not 0 <= S <= S_cap or offsets[S] > cap:
        raise _native.NativeError(f"label_maps_to_rle: {S} segments of {S_cap}, {offsets[S]} characters of {cap}")
    raw = host[head + hdr_bytes:head + hdr_bytes + offsets[S]].tobytes()
    found = [[] for _ in range(B)]
    for s in range(S):
        i, label, area, x0, y0, x1, y1, n = headers[s].tolist()
        if not 0 <= i < B or n != pixels[i]:
            raise _native.NativeError(f"label_maps_to_rle: segment {s} names image {i} of {n} pixels")
        rle = {"size": [int(hw[i, 0]), int(hw[i, 1])], "counts": raw[offsets[s]:offsets[s + 1]].decode("ascii")}
        found[i].append(_entry(label, rle, area, (x0, y0, x1 - x0 + 1, y1 - y0 + 1)))
    if ids is None:
        return found
    out_lists = []
    for i, one in enumerate(ids):
        by_label = {e["label"]: e for e in found[i]}
        H, W = int(hw[i, 0]), int(hw[i, 1])
        out_lists.append([dict(by_label[v]) if v in by_label else _empty_entry(v, H, W) for v in one])
    return out_lists


def label_maps_to_rle(planes, *, ignore=None, ids=None):
    """planes: one (H_i, W_i) label plane per image, uint8, int16 or int32 (one dtype and one device per batch; sizes
    may differ; a row-strided crop view is read in place).  ``ignore``: a value, or one per image, whose pixels belong
    to no segment.  ``ids=None``: every distinct value but ``ignore`` in ascending signed order (``np.unique``);
    ``ids=[[...], ...]``: per image exactly those values in that order, a value without pixels giving the all-zero RLE,
    area 0 and box ``[0, 0, 0, 0]``.

    -> per image a list of ``{"label": int, "segmentation": {"size": [H, W], "counts": str}, "area": int,
    "bbox": [xmin, ymin, w, h]}``.  A plane of zero pixels yields no segments.  ``H * W`` must stay below 2^31."""
    planes = _check_planes(planes)
    B = len(planes)
    ignores = _per_image(ignore, B, "ignore values")
    ids = _id_lists(ids, B)
    if B == 0:
        return []
    if planes[0].device.type != "cuda":
        return [_segments_host(p.numpy(), ignores[i], None if ids is None else ids[i]) for i, p in enumerate(planes)]
    live = [i for i, p in enumerate(planes) if p.numel()]
    out = [[] for _ in range(B)]
    if live:
        got = _segments_device([planes[i] for i in live], [ignores[i] for i in live],
                               None if ids is None else [ids[i] for i in live])
        for i, one in zip(live, got):
            out[i] = one
    return out


# -------------------------------------------------------------------------------------------------------------------
# the inverse
# -------------------------------------------------------------------------------------------------------------------
def _decode_one(rle):
    """RLE dict (compressed or the uncompressed list) -> (H, W) bool numpy."""
    if isinstance(rle["counts"], (str, bytes)):
        return rle_decode(rle).numpy()
    H, W = rle["size"]
    counts = np.asarray(rle["counts"], dtype=np.int64).reshape(-1)
    return np.repeat(np.arange(counts.size) % 2 == 1, counts).reshape(W, H).T


def rle_to_label_maps(segments, sizes, *, fill=0, dtype=torch.int32, device=None):
    """segments: per image a list of ``(value, rle)``, ``rle`` a dict with a compressed string, bytes or the
    uncompressed list of counts (the forms of :func:`rle_to_bits_ragged`); sizes: the (H, W) of every image.  Every
    plane starts as ``fill`` and the segments are painted in list order, a later one overwriting an earlier one
    (``segm_dt[mask > 0] = category_id``).  -> one (H, W) plane of ``dtype`` (uint8, int16 or int32) per image on
    ``device``; on a HIP device one upload and one launch of ``m2f_rle_paint_labels``.

    Raises ValueError, before any launch, for a segment whose size is not its image's, counts that do not add up, a
    malformed string, and a value or ``fill`` that does not fit ``dtype``."""
    device = torch.device("cpu" if device is None else device)
    if dtype not in LABEL_DTYPES:
        raise ValueError(f"dtype must be uint8, int16 or int32, got {dtype}")
    nbytes, lo, hi = LABEL_DTYPES[dtype]
    segments = [list(one) for one in segments]
    sizes = [(int(s[0]), int(s[1])) for s in sizes]
    if len(sizes) != len(segments):
        raise ValueError(f"{len(sizes)} sizes for {len(segments)} images")
    fill = int(fill)
    if not lo <= fill <= hi:
        raise ValueError(f"fill {fill} does not fit {dtype}")
    rles, values, owner_pixels = [], [], []
    for i, (one, (H, W)) in enumerate(zip(segments, sizes)):
        if H < 0 or W < 0 or H * W >= 2 ** 31:
            raise ValueError(f"image {i}: {H} x {W} pixels: sizes must fit a 32-bit count")
        for value, rle in one:
            if [int(v) for v in rle["size"]] != [H, W]:
                raise ValueError(f"image {i}: a segment of size {list(rle['size'])} in an image of {[H, W]}")
            if not lo <= int(value) <= hi:
                raise ValueError(f"image {i}: the value {int(value)} does not fit {dtype}")
            rles.append(rle)
            values.append(int(value))
            owner_pixels.append(H * W)
    B = len(sizes)
    if B == 0:
        return []
    if rles:
        positions, offsets = _run_ends_chunked(rles, np.array(owner_pixels, dtype=np.int64))   # every check of counts
    else:
        positions, offsets = np.zeros(0, np.int32), np.zeros(1, np.int64)
    if device.type != "cuda":
        planes = []
        for one, (H, W) in zip(segments, sizes):
            plane = np.full((H, W), fill, dtype=np.int64)
            for value, rle in one:
                plane[_decode_one(rle)] = int(value)
            planes.append(torch.from_numpy(plane).to(dtype).to(device))
        return planes
    hw = np.array(sizes, dtype=np.int64).reshape(B, 2)
    nseg = np.array([len(one) for one in segments], dtype=np.int64)
    seg0 = np.concatenate(([0], np.cumsum(nseg)))
    elems = hw[:, 0] * hw[:, 1]
    out_off = np.concatenate(([0], np.cumsum(elems)))
    block_base = np.concatenate(([0], np.cumsum(((hw[:, 1] + 63) // 64) * ((hw[:, 0] + 3) // 4))))
    images = np.stack((hw[:, 0], hw[:, 1], seg0[:-1], seg0[1:], out_off[:-1], block_base[:-1]), axis=1).astype(np.int64)
    t = _native.upload_tables({"offsets": offsets, "images": images, "positions": positions,
                               "values": np.array(values, dtype=np.int32)}, device)  # the one upload
    out = torch.empty(int(out_off[-1]), dtype=dtype, device=device)
    if int(block_base[-1]):
        with torch.cuda.device(device):
            _native.call("m2f_rle_paint_labels", _native.ptr_or_null(t["positions"]), t["positions"].numel(),
                         t["offsets"].data_ptr(), len(rles), _native.ptr_or_null(t["values"]), t["images"].data_ptr(),
                         B, int(block_base[-1]), fill, nbytes, out.data_ptr(), out.numel(), _native.stream(device))
    return [out[a:b].view(H, W) for a, b, (H, W) in zip(out_off[:-1].tolist(), out_off[1:].tolist(), sizes)]
