"""Label-pair counts: for an image with a ground-truth label plane ``a`` and a predicted label plane ``b``, the number
of pixels of every (row of a, column of b) pair.  Semantic mIoU reads them as one confusion matrix accumulated over a
dataset (what detectron2's ``SemSegEvaluator`` gets from ``np.bincount`` on host copies), panoptic PQ as one table of
ground-truth segment x predicted segment per image (what panopticapi gets from ``np.unique`` on a combined 64-bit
map read back from PNG files).

:func:`label_pair_counts_ragged`  a batch of images of any sizes: one upload of the small tables, one launch of
                                  ``m2f_label_pair_counts_ragged`` (``csrc/label_counts.hip``) and one copy of the
                                  tables to the host.
:func:`label_pair_counts`         the single-image form.
:func:`label_histogram_ragged`    the counts of one plane alone, per image (``m2f_label_histogram_ragged``, the same
                                  kernel without the plane ``b``): which classes an image holds and their areas.

The row of a value ``v`` of ``a``:

direct mode (``ids=None``)  ``v == ignore`` -> the last row, ``rows - 1`` (tested first); ``v`` in ``[0, rows - 1)``
                            -> row ``v``; any other value adds one to the image's ``bad`` count and the pixel is not
                            counted.
id-list mode                the image has a sorted list of up to ``MAX_IDS`` int32 ids; ``v`` found at index ``j`` ->
                            row ``j``; ``v`` not in the list -> the last row ("other").

The column of a value ``w`` of ``b``: ``w`` in ``[0, cols)`` -> column ``w``; any other value is ``bad``.

The device counters are 64-bit, so every batch that fits the device is counted exactly and nothing is refused for its
size.  On CPU tensors and numpy arrays the same definition runs in numpy (``np.searchsorted`` and ``np.bincount``);
that is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native
from .label_planes import np_dtype, reads

_PATHS = {"auto": 0, "lds": 1, "global": 2}
_FIELDS = 8                               # M2F_LABEL_IMAGE_FIELDS
_geometry = None


def geometry():
    """(vec, chunk_vecs, lds_bins, max_ids) of ``csrc/label_counts.hip``: pixels per lane and load, vectors per
    workgroup, the counters the LDS path can hold and the longest id list."""
    global _geometry
    if _geometry is None:
        _geometry = _native.query("m2f_label_counts_geometry", outs="iiii")
    return _geometry


MAX_IDS = 1024                            # M2F_LABEL_MAX_IDS
_INT_MAX = 2 ** 31 - 1


def _dtype(p):
    return np_dtype(p.dtype if torch.is_tensor(p) else np.asarray(p).dtype)


def _per_image(value, n, name):
    if np.ndim(value) == 0:
        return np.full(n, int(value), dtype=np.int64)
    out = np.asarray(value, dtype=np.int64).reshape(-1)
    if out.size != n:
        raise ValueError(f"{out.size} values of {name} for {n} images")
    return out


def _plan(a_planes, b_planes, rows, cols, ignore, ids, share_output, path):
    """Every check of label_pair_counts_ragged -> a dict of the batch's host-side description (no device work)."""
    a_planes, b_planes = list(a_planes), list(b_planes)
    G = len(a_planes)
    if len(b_planes) != G:
        raise ValueError(f"{G} planes of a and {len(b_planes)} of b")
    if path not in _PATHS:
        raise ValueError(f"path {path!r} is not one of {sorted(_PATHS)}")
    rows, cols = _per_image(rows, G, "rows"), _per_image(cols, G, "cols")
    if ((rows < 1) | (cols < 1)).any() or (rows * cols > _INT_MAX).any():
        raise ValueError("rows and cols must be positive and rows * cols fit 31 bits")
    if ids is not None and ignore is not None:
        raise ValueError("ignore belongs to the direct mode; with ids the last row collects what is not listed")
    if ignore is not None and not -2 ** 31 <= int(ignore) < 2 ** 31:
        raise ValueError("ignore must fit an int32")
    id_lists = None
    if ids is not None:
        id_lists = [np.asarray(x, dtype=np.int64).reshape(-1) for x in ids]
        if len(id_lists) != G:
            raise ValueError(f"{len(id_lists)} id lists for {G} images")
        for i, x in enumerate(id_lists):
            if x.size > MAX_IDS or x.size > rows[i] - 1:
                raise ValueError(f"image {i}: {x.size} ids, at most min({MAX_IDS}, rows - 1 = {rows[i] - 1}) fit")
            if x.size and (x.min() < -2 ** 31 or x.max() >= 2 ** 31):
                raise ValueError(f"image {i}: ids must fit an int32")
            if (np.diff(x) <= 0).any():
                raise ValueError(f"image {i}: ids must be sorted ascending without repeats")
    if share_output and G and ((rows != rows[0]).any() or (cols != cols[0]).any()):
        raise ValueError("share_output needs one table size for all images")
    pixels = np.zeros(G, dtype=np.int64)
    a_dt = b_dt = None
    kinds = set()
    for i, (a, b) in enumerate(zip(a_planes, b_planes)):
        da, db = _dtype(a), _dtype(b)
        if not reads(da) or not reads(db, wide=True):
            raise ValueError(f"image {i}: a must be uint8, int16 or int32 and b uint8, int16, int32 or int64, got "
                             f"{da} and {db}")
        if (a_dt, b_dt) != (None, None) and (da, db) != (a_dt, b_dt):
            raise ValueError(f"image {i}: planes of {da} / {db} in a batch of {a_dt} / {b_dt}")
        a_dt, b_dt = da, db
        na = a.numel() if torch.is_tensor(a) else np.asarray(a).size
        nb = b.numel() if torch.is_tensor(b) else np.asarray(b).size
        if na != nb:
            raise ValueError(f"image {i}: a has {na} pixels and b {nb}")
        pixels[i] = na
        for p in (a, b):
            kinds.add(str(p.device) if torch.is_tensor(p) and p.device.type == "cuda" else "host")
    devices = kinds - {"host"}
    if len(devices) > 1:
        raise ValueError(f"planes on several devices: {sorted(devices)}")
    bins = rows * cols
    out_off = np.zeros(G, dtype=np.int64) if share_output else np.concatenate(([0], np.cumsum(bins)))[:-1]
    out_len = int(bins[0]) if share_output and G else int(bins.sum())
    return {"a": a_planes, "b": b_planes, "G": G, "rows": rows, "cols": cols, "pixels": pixels, "ids": id_lists,
            "ignore": None if ignore is None else int(ignore), "share": bool(share_output), "path": path,
            "out_off": out_off.astype(np.int64), "out_len": out_len, "a_dtype": a_dt, "b_dtype": b_dt,
            "device": torch.device(devices.pop()) if devices else None}


# -------------------------------------------------------------------------------------------------------------------
# the definition, in numpy
# -------------------------------------------------------------------------------------------------------------------
def _host(p):
    return (p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)).reshape(-1)


def _counts_host(plan):
    out = np.zeros(plan["out_len"], dtype=np.int64)
    bad = np.zeros(plan["G"], dtype=np.int64)
    for i in range(plan["G"]):
        a, b = _host(plan["a"][i]).astype(np.int64), _host(plan["b"][i]).astype(np.int64)
        rows, cols = int(plan["rows"][i]), int(plan["cols"][i])
        if plan["ids"] is None:
            row = np.where((a >= 0) & (a < rows - 1), a, -1)
            if plan["ignore"] is not None:
                row = np.where(a == plan["ignore"], rows - 1, row)
        else:
            ids = plan["ids"][i]
            padded = np.concatenate((ids, [np.iinfo(np.int64).max]))           # searchsorted may answer ids.size
            j = np.searchsorted(ids, a)
            row = np.where(padded[j] == a, j, rows - 1)
        good = (row >= 0) & (b >= 0) & (b < cols)
        bad[i] = a.size - int(good.sum())
        o = int(plan["out_off"][i])
        out[o:o + rows * cols] += np.bincount(row[good] * cols + b[good], minlength=rows * cols)
    return out, bad


# -------------------------------------------------------------------------------------------------------------------
# the device route
# -------------------------------------------------------------------------------------------------------------------
def _gather(planes, np_dtype, device, align):
    """Planes of one side -> (base pointer, element offsets (G,), elements spanned, keep-alive).  Contiguous device
    planes are read where they lie; a non-contiguous one (a crop ``out[b, :h, :w]`` of a wider batch buffer) is first
    made contiguous on the device.  The base is the lowest plane address rounded down to 16 bytes and the offsets are
    counted from it, so the kernel's aligned loads are available whatever the first plane's own alignment; nothing
    is read between the base and the first plane.  Host planes are concatenated, each on a multiple of ``align``
    elements, and uploaded in one copy."""
    G = len(planes)
    item = np.dtype(np_dtype).itemsize
    tdtype = getattr(torch, np.dtype(np_dtype).name)
    keep, ptrs, sizes = [], np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    host_idx = [i for i, p in enumerate(planes) if not (torch.is_tensor(p) and p.device.type == "cuda")]
    if host_idx:
        parts, at, starts = [], 0, []
        for i in host_idx:
            flat = _host(planes[i])
            starts.append(at)
            pad = -flat.size % align
            parts.append(flat)
            if pad:
                parts.append(np.zeros(pad, dtype=np_dtype))
            at += flat.size + pad
        buf = torch.from_numpy(np.concatenate(parts) if at else np.zeros(align, dtype=np_dtype)).to(device)  # one copy
        keep.append(buf)
        for i, s in zip(host_idx, starts):
            ptrs[i] = buf.data_ptr() + s * item
    for i, p in enumerate(planes):
        sizes[i] = p.numel() if torch.is_tensor(p) else np.asarray(p).size
        if i in host_idx:
            continue
        t = p.detach()
        if t.dtype != tdtype:
            raise ValueError("plane dtype changed under the plan")
        if not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        ptrs[i] = t.data_ptr()
    live = sizes > 0
    if not live.any():
        return 0, np.zeros(G, dtype=np.int64), 0, keep
    base = int(ptrs[live].min()) // 16 * 16                           # item divides 16 and every plane address
    off = np.where(live, (ptrs - base) // item, 0)
    return base, off.astype(np.int64), int((off + sizes)[live].max()), keep


def _blocks(a_off, pixels):
    vec, chunk_vecs = geometry()[:2]
    nvec = np.where(pixels > 0, (a_off % vec + pixels + vec - 1) // vec, 0)
    nblk = (nvec + chunk_vecs - 1) // chunk_vecs
    image_of = np.repeat(np.arange(pixels.size, dtype=np.int64), nblk)
    first = np.concatenate(([0], np.cumsum(nblk)))[:-1]
    return np.stack((image_of, np.arange(image_of.size) - first[image_of]), axis=1).astype(np.int32)


def _counts_device(plan):
    device = plan["device"]
    G = plan["G"]
    vec, _, lds_bins, _ = geometry()
    max_bins = int((plan["rows"] * plan["cols"]).max())
    if plan["path"] == "lds" and max_bins > lds_bins:
        raise ValueError(f"path='lds': a table of {max_bins} counters is beyond the {lds_bins} the LDS path holds")
    with torch.cuda.device(device):
        a_base, a_off, a_elems, keep_a = _gather(plan["a"], plan["a_dtype"], device, 2 * vec)
        b_base, b_off, b_elems, keep_b = _gather(plan["b"], plan["b_dtype"], device, 2 * vec)
        ids = plan["ids"]
        id_n = np.full(G, -1, dtype=np.int64) if ids is None else np.array([x.size for x in ids], dtype=np.int64)
        id_off = np.zeros(G, dtype=np.int64) if ids is None else np.concatenate(([0], np.cumsum(id_n)))[:-1]
        images = np.stack((a_off, b_off, plan["pixels"], plan["rows"], plan["cols"], plan["out_off"], id_off, id_n),
                          axis=1).astype(np.int64)
        assert images.shape[1] == _FIELDS
        blocks = _blocks(a_off, plan["pixels"])
        flat_ids = (np.concatenate(ids) if ids else np.zeros(0, np.int64)).astype(np.int32)
        dev = _native.upload_tables({"images": images, "ids": flat_ids, "blocks": blocks}, device)  # one copy
        out = torch.zeros(plan["out_len"] + G, dtype=torch.int64, device=device)
        ign = plan["ignore"]
        _native.call("m2f_label_pair_counts_ragged", a_base or None, plan["a_dtype"].itemsize, a_elems, b_base or None,
                     plan["b_dtype"].itemsize, b_elems, dev["images"].data_ptr(), G, _native.ptr_or_null(dev["ids"]),
                     flat_ids.size, _native.ptr_or_null(dev["blocks"]), blocks.shape[0], int(ign is not None), ign or 0,
                     max_bins, _PATHS[plan["path"]], out.data_ptr(), plan["out_len"],
                     out.data_ptr() + 8 * plan["out_len"], _native.stream(device))
        host = out.cpu().numpy()                                                                  # the one copy
    del keep_a, keep_b
    return host[:plan["out_len"]], host[plan["out_len"]:]


def label_pair_counts_ragged(a_planes, b_planes, *, rows, cols, ignore=None, ids=None, share_output=False,
                             path="auto"):
    """a_planes, b_planes: one ground-truth and one predicted label plane per image (any shape, read flat; the two of
    an image hold the same number of pixels, which may be zero).  ``a`` is uint8, int16 or int32 and ``b`` uint8,
    int16, int32 or int64, one dtype per side for the whole batch.  ``rows`` and ``cols`` are the table size, one
    int or one per image; ``ignore`` and ``ids`` (one sorted list of distinct int32 ids per image) choose the row
    mapping described in the module's docstring.

    -> ``(tables, bad)``: ``tables`` a list of host int64 arrays ``(rows_i, cols_i)``, or with ``share_output`` the one
    table all images were added into; ``bad`` (G,) int64, the pixels of each image that map to no row or column.

    If any plane is a HIP tensor the batch is counted on its device: contiguous device planes are read where they
    lie (a non-contiguous view, such as a crop of a wider buffer, is made contiguous on the device first), host
    planes (numpy arrays or CPU tensors) go up in one concatenated copy per side.  ``path`` forces the kernel's LDS
    or global-atomic path (``"lds"`` raises ValueError when a table is beyond :func:`geometry`'s ``lds_bins``); the
    counts do not depend on it.  With only host planes the numpy definition runs."""
    plan = _plan(a_planes, b_planes, rows, cols, ignore, ids, share_output, path)
    G = plan["G"]
    if G == 0:
        shared = np.zeros((int(rows), int(cols)) if np.ndim(rows) == 0 and np.ndim(cols) == 0 else (0, 0), np.int64)
        return (shared if share_output else []), np.zeros(0, np.int64)
    flat, bad = _counts_host(plan) if plan["device"] is None else _counts_device(plan)
    if share_output:
        return flat.reshape(int(plan["rows"][0]), int(plan["cols"][0])).copy(), bad.copy()
    tables = [flat[o:o + r * c].reshape(r, c).copy()
              for o, r, c in zip(plan["out_off"], plan["rows"], plan["cols"])]
    return tables, bad.copy()


def label_pair_counts(a, b, *, rows, cols, ignore=None, ids=None, path="auto"):
    """One image: -> ``(table (rows, cols) int64, bad)``; see :func:`label_pair_counts_ragged`."""
    tables, bad = label_pair_counts_ragged([a], [b], rows=rows, cols=cols, ignore=ignore,
                                           ids=None if ids is None else [ids], path=path)
    return tables[0], int(bad[0])


def label_histogram_ragged(planes, bins, ignore=None, *, path="auto"):
    """planes: one label plane per image (uint8, int16 or int32, one dtype for the batch; any shape, read flat, may be
    empty).  -> ``(counts, bad)`` on the host: ``counts`` (B, bins + 1) int64, column ``v < bins`` the pixels of value
    ``v`` and column ``bins`` the pixels equal to ``ignore`` (0 without one; ``ignore`` is tested first); ``bad`` (B,)
    int64, the pixels that are neither.

    If any plane is a HIP tensor: one upload of the small tables, one launch of ``m2f_label_histogram_ragged`` over
    the whole batch and one copy to the host, planes read in place as by :func:`label_pair_counts_ragged` (``path``
    as there).  With only host planes the numpy definition (``np.bincount``) runs."""
    planes = list(planes)
    B, bins = len(planes), int(bins)
    if path not in _PATHS:
        raise ValueError(f"path {path!r} is not one of {sorted(_PATHS)}")
    if not 1 <= bins < _INT_MAX:
        raise ValueError("bins must be positive and bins + 1 fit 31 bits")
    if ignore is not None and not -2 ** 31 <= int(ignore) < 2 ** 31:
        raise ValueError("ignore must fit an int32")
    rows = bins + 1
    dt, devices = None, set()
    for i, p in enumerate(planes):
        d = _dtype(p)
        if not reads(d) or (dt is not None and d != dt):
            raise ValueError(f"image {i}: planes must be uint8, int16 or int32, one dtype per batch, got {d}"
                             + (f" after {dt}" if dt is not None else ""))
        dt = d
        if torch.is_tensor(p) and p.device.type == "cuda":
            devices.add(str(p.device))
    if len(devices) > 1:
        raise ValueError(f"planes on several devices: {sorted(devices)}")
    if B == 0:
        return np.zeros((0, rows), np.int64), np.zeros(0, np.int64)
    if not devices:
        counts, bad = np.zeros((B, rows), np.int64), np.zeros(B, np.int64)
        for i, p in enumerate(planes):
            a = _host(p).astype(np.int64)
            row = np.where((a >= 0) & (a < bins), a, -1)
            if ignore is not None:
                row = np.where(a == int(ignore), bins, row)
            bad[i] = int((row < 0).sum())
            counts[i] = np.bincount(row[row >= 0], minlength=rows)
        return counts, bad
    device = torch.device(devices.pop())
    vec, _, lds_bins, _ = geometry()
    if path == "lds" and rows > lds_bins:
        raise ValueError(f"path='lds': a table of {rows} counters is beyond the {lds_bins} the LDS path holds")
    with torch.cuda.device(device):
        base, off, elems, keep = _gather(planes, dt, device, 2 * vec)
        pixels = np.array([p.numel() if torch.is_tensor(p) else np.asarray(p).size for p in planes], dtype=np.int64)
        one, none = np.ones(B, np.int64), np.zeros(B, np.int64)
        images = np.stack((off, none, pixels, rows * one, one, rows * np.arange(B, dtype=np.int64), none, -one),
                          axis=1).astype(np.int64)
        assert images.shape[1] == _FIELDS
        blocks = _blocks(off, pixels)
        dev = _native.upload_tables({"images": images, "blocks": blocks}, device)                # one copy
        out = torch.zeros(B * rows + B, dtype=torch.int64, device=device)
        _native.call("m2f_label_histogram_ragged", base or None, dt.itemsize, elems, dev["images"].data_ptr(), B,
                     _native.ptr_or_null(dev["blocks"]), blocks.shape[0], int(ignore is not None), int(ignore or 0),
                     rows, _PATHS[path], out.data_ptr(), B * rows, out.data_ptr() + 8 * B * rows,
                     _native.stream(device))
        host = out.cpu().numpy()                                                                  # the one copy
    del keep
    return host[:B * rows].reshape(B, rows).copy(), host[B * rows:].copy()
