"""COCO polygon segmentations -> bit planes and RLE: what the reference's mappers and evaluators get from
``pycocotools.mask.frPyObjects`` / ``merge`` and ``polygons_to_bitmask`` (mask2former/data/dataset_mappers/
coco_instance_new_baseline_dataset_mapper.py:22-23,185, mask_former_instance_dataset_mapper.py:128,
mask2former_video/data_video/datasets/ytvis_api/ytvos.py:262-280), restated without pycocotools.

The rasteriser is ``rleFrPoly`` of pycocotools' ``maskApi.c`` restated as a definition (DESIGN.md §3 gives it in
full).  pycocotools itself has never been run against this code; what is tested is the definition.

  1. A polygon of k >= 3 points (x, y) in fp64 becomes integer vertices ``X = trunc(5 x + 0.5)``, ``Y`` likewise,
     closed by its first point.
  2. An edge is *flat* when ``|dX| >= |dY|`` and *steep* otherwise.  Oriented along its long axis it is the points
     ``(xs + t, trunc(ys + s t + 0.5))`` (flat, ``s = dY / dX``) or ``(trunc(xs + s t + 0.5), ys + t)`` (steep,
     ``s = dX / dY``), ``t = 0 .. max(|dX|, |dY|)``; every fp64 operation is rounded on its own (no FMA).
  3. Two consecutive points whose x differ give a *crossing* at the smaller x ``u`` when ``u - 2`` is divisible by 5
     and the column ``c = (u - 2) / 5`` lies in the image; with ``v`` the smaller y its row is
     ``clamp(ceil((v - 2) / 5), 0, H)`` and its position ``p = c H + row``.  An edge's kept crossings are exactly the
     ``u = 5 c + 2`` in ``[min(xs, xe), max(xs, xe) - 1]``, so their number is known without walking the edge.
  4. Pixel ``q = x H + y`` (column-major) is set when an odd number of positions is ``<= q``.
  5. An annotation is the OR of its polygons; ``[]`` is the zero mask.

:func:`polygon_crossings`        the sorted positions of every polygon (with the closing sentinel ``H W``).
:func:`polygons_to_bits_ragged`  annotations of images of any sizes -> one flat word buffer in the layout of
                                 ``rle_to_bits_ragged``, which ``mask_pair_counts_ragged`` reads unchanged.
:func:`polygons_to_bits`         annotations of one size -> (M, H, ceil(W / 32)) planes as ``rle_to_bits`` gives.
:func:`polygons_to_rle`, :func:`ann_to_rle`, :func:`convert_polygons_to_rle`
                                 ``frPyObjects``, ``COCO.annToRLE`` and a whole instances file, through the planes
                                 and ``rle_encode``.
:func:`pair_counts_ragged`       the evaluator's batch step for RLE masks and polygon annotations in one buffer.

On a HIP device the host does O(vertices) vectorised work (integer vertices, the per-edge crossing counts and the
tables, one upload); ``m2f_poly_crossings`` evaluates one crossing per thread, one ``torch.sort`` orders the batch
and ``m2f_poly_decode_bits_ragged`` writes the planes (``csrc/polygon.hip``).  On a CPU device a vectorised numpy
restatement of the same rules runs; that is not a fallback: on a HIP device a kernel error raises ``NativeError``.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import _native
from .mask_iou import (_PLANE_ALIGN, MAX_RAGGED_WORDS, _check_size, _decode_plan, _groups_by_offset, _launch_decode,
                       _launch_pairs, _pack_rows, _pair_counts_ragged_host, _pair_plan, _plane_words, _split_counts,
                       rle_pair_counts_ragged, rle_to_bits_ragged)
from .rle import counts_to_string, rle_encode

MAX_COORD = 2.0 ** 26                   # |x|, |y| below this keep 5 x + 0.5 and the edge lengths inside int32
_EDGE_FIELDS = 8                        # M2F_POLY_EDGE_FIELDS: kind, xs, ys, steps, c0, H, W, polygon
_FLAT, _STEEP, _SENTINEL = 0, 1, 2
DEFAULT_BATCH_BYTES = 64 << 20          # planes per batch of convert_polygons_to_rle, as the evaluator's


# -------------------------------------------------------------------------------------------------------------------
# checks and tables (host, O(vertices))
# -------------------------------------------------------------------------------------------------------------------
def check_annotation(polys, name="the annotation"):
    """A polygon segmentation (a list of flat ``[x0, y0, x1, y1, ...]`` lists) -> its polygons as float64 arrays.
    Raises ValueError naming ``name`` for a polygon with an odd number of values or fewer than 6, non-finite
    coordinates or ``|coordinate| >= 2^26``."""
    if isinstance(polys, dict) or isinstance(polys, (str, bytes)) or not hasattr(polys, "__len__"):
        raise ValueError(f"{name}: a polygon segmentation must be a list of polygons")
    out = []
    for i, p in enumerate(polys):
        try:
            a = np.asarray(p, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{name}: polygon {i} is not a flat list of numbers") from e
        if a.ndim != 1:
            raise ValueError(f"{name}: polygon {i} is not a flat list of numbers")
        if a.size % 2 or a.size < 6:
            raise ValueError(f"{name}: polygon {i} has {a.size} values; an even number of at least 6 is needed")
        if not np.isfinite(a).all():
            raise ValueError(f"{name}: polygon {i} has non-finite coordinates")
        if (np.abs(a) >= MAX_COORD).any():
            raise ValueError(f"{name}: polygon {i} has a coordinate of magnitude 2^26 or more")
        out.append(a)
    return out


def _sizes(sizes, n, what):
    """-> (n, 2) int64 (H, W): one pair for all, or one per entry."""
    hw = np.asarray(sizes, dtype=np.int64)
    if hw.ndim == 1 and hw.size == 2:
        hw = np.broadcast_to(hw, (n, 2))
    if hw.shape != (n, 2):
        raise ValueError(f"sizes of shape {hw.shape} for {n} {what}: one (H, W) each is needed")
    return np.ascontiguousarray(hw)


class _Plan:
    """The host tables of a batch of annotations: ``edges`` / ``slopes`` / ``starts`` as ``m2f_poly_crossings``
    takes them (include/bm2f.h), ``pos_offsets`` (P + 1) and ``part_offsets`` (A + 1)."""


def _plan(anns, hw, names=None) -> _Plan:
    """Every check of the polygon entry points, then rules 1 and 2 and the closed-form counts of rule 3."""
    A = len(anns)
    names = names if names is not None else [f"annotation {m}" for m in range(A)]
    for m in range(A):
        _check_size(int(hw[m, 0]), int(hw[m, 1]), f"{names[m]}: ")
    parts = [check_annotation(a, names[m]) for m, a in enumerate(anns)]
    nparts = np.array([len(p) for p in parts], dtype=np.int64)
    polys = [p for ps in parts for p in ps]
    P = len(polys)
    poly_hw = np.repeat(hw, nparts, axis=0).reshape(P, 2)
    k = np.array([p.size // 2 for p in polys], dtype=np.int64)
    xy = np.concatenate(polys).reshape(-1, 2) if P else np.zeros((0, 2))
    V = int(k.sum())
    # rule 1
    X = np.trunc(5.0 * xy[:, 0] + 0.5).astype(np.int64)
    Y = np.trunc(5.0 * xy[:, 1] + 0.5).astype(np.int64)
    first = np.repeat(np.concatenate(([0], np.cumsum(k)))[:-1], k)
    idx = np.arange(V)
    nxt = first + (idx - first + 1) % np.repeat(k, k)
    owner = np.repeat(np.arange(P), k)
    # rule 2: orientation and slope
    xs, ys, xe, ye = X, Y, X[nxt], Y[nxt]
    dx, dy = np.abs(xe - xs), np.abs(ye - ys)
    flat = dx >= dy
    flip = np.where(flat, xs > xe, ys > ye)
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    steps = np.where(flat, dx, dy)
    num = np.where(flat, ye - ys, xe - xs).astype(np.float64)
    slope = np.divide(num, steps.astype(np.float64), out=np.zeros(V), where=steps > 0)
    # rule 3: the kept columns of an edge are those with 5 c + 2 in [min x, max x - 1], inside the image
    W_e = poly_hw[owner, 1] if V else np.zeros(0, np.int64)
    c_lo = np.maximum(-((2 - np.minimum(xs, xe)) // 5), 0)           # ceil((min x - 2) / 5)
    c_hi = np.minimum((np.maximum(xs, xe) - 3) // 5, W_e - 1)
    count = np.maximum(c_hi - c_lo + 1, 0)
    E = V + P                                                        # every polygon's sentinel is one more row
    edges = np.zeros((E, _EDGE_FIELDS), dtype=np.int64)
    edges[:V, 0] = np.where(flat, _FLAT, _STEEP)
    edges[:V, 1], edges[:V, 2], edges[:V, 3], edges[:V, 4] = xs, ys, steps, np.minimum(c_lo, 2 ** 31 - 1)
    edges[:V, 5:7] = poly_hw[owner] if V else 0
    edges[:V, 7] = owner
    edges[V:, 0] = _SENTINEL
    edges[V:, 5:7] = poly_hw
    edges[V:, 7] = np.arange(P)
    count = np.concatenate((count, np.ones(P, np.int64)))
    plan = _Plan()
    plan.edges = edges.astype(np.int32)
    plan.slopes = np.concatenate((slope, np.zeros(P)))
    plan.starts = np.concatenate(([0], np.cumsum(count)))[:-1].astype(np.int64)
    plan.counts = count
    plan.total = int(count.sum())
    if plan.total >= 2 ** 31:
        raise ValueError(f"the batch has {plan.total} crossings, more than the 2^31 - 1 of one call; split it")
    per_poly = np.bincount(edges[:, 7], weights=count, minlength=P).astype(np.int64) if E else np.zeros(0, np.int64)
    plan.pos_offsets = np.concatenate(([0], np.cumsum(per_poly))).astype(np.int64)
    plan.part_offsets = np.concatenate(([0], np.cumsum(nparts))).astype(np.int64)
    plan.num_polys, plan.num_anns, plan.hw = P, A, np.ascontiguousarray(hw, dtype=np.int64)
    return plan


def _line(a, s, t):
    """trunc(a + s * t + 0.5), every operation rounded on its own (numpy does not contract)."""
    prod = s * t.astype(np.float64)
    return np.trunc((a.astype(np.float64) + prod) + 0.5).astype(np.int64)


def _crossings_host(plan):
    """Rule 3 for every kept crossing at once -> the sorted positions (total,) int32, polygon after polygon."""
    d, n = plan.edges.astype(np.int64), plan.counts
    e = np.repeat(np.arange(d.shape[0]), n)
    j = np.arange(plan.total) - np.repeat(plan.starts, n)
    kind, xs, ys, steps, H, W = d[e, 0], d[e, 1], d[e, 2], d[e, 3], d[e, 5], d[e, 6]
    s = plan.slopes[e]
    c = d[e, 4] + j
    u = 5 * c + 2
    t = u - xs
    v_flat = np.minimum(_line(ys, s, t), _line(ys, s, t + 1))
    a, b = np.zeros_like(steps), steps.copy()                        # bisection over the steps of a steep edge
    steep = kind == _STEEP
    for _ in range(32):
        active = steep & (b - a > 1)
        if not active.any():
            break
        mid = (a + b) >> 1
        x = _line(xs, s, mid)
        near = np.where(s > 0, x <= u, x >= u + 1)
        a = np.where(active & near, mid, a)
        b = np.where(active & ~near, mid, b)
    v = np.where(steep, ys + a, v_flat)
    row = np.where(v <= 2, 0, np.minimum((v + 2) // 5, H))           # ceil((v - 2) / 5) clamped to [0, H]
    p = np.where(kind == _SENTINEL, H * W, c * H + row)
    keys = np.sort((d[e, 7] << 32) | p)
    return (keys & 0x7fffffff).astype(np.int32)


def _decode_host(positions, plan, out_offsets, total_words):
    """Rules 4 and 5 -> the flat word buffer (padding words zero)."""
    words = np.zeros(total_words, dtype=np.int32)
    for m, (H, W) in enumerate(plan.hw):
        mask = np.zeros(H * W, dtype=bool)
        for q in range(plan.part_offsets[m], plan.part_offsets[m + 1]):
            t = positions[plan.pos_offsets[q]:plan.pos_offsets[q + 1]]
            flips = np.bincount(t[t < H * W], minlength=H * W)
            mask |= (np.cumsum(flips) & 1).astype(bool)
        plane = _pack_rows(mask.reshape(W, H).T)
        words[out_offsets[m]:out_offsets[m] + plane.size] = plane.reshape(-1)
    return words


# -------------------------------------------------------------------------------------------------------------------
# device path
# -------------------------------------------------------------------------------------------------------------------
def _blocks(hw):
    """(annotation, block of 256 columns) rows, ceil(W / 256) per annotation."""
    nblk = (hw[:, 1] + 255) // 256
    ann_of = np.repeat(np.arange(hw.shape[0], dtype=np.int64), nblk)
    first = np.concatenate(([0], np.cumsum(nblk)))[:-1]
    return np.stack((ann_of, np.arange(ann_of.size) - first[ann_of]), axis=1).astype(np.int32)


def _tables(plan, out_offsets):
    """The arrays both kernels read, named so that they can share an upload with the RLE and pair tables."""
    return {"poly_slopes": plan.slopes.view(np.int64), "poly_starts": plan.starts,
            "poly_pos_offsets": plan.pos_offsets, "poly_part_offsets": plan.part_offsets,
            "poly_out_offsets": np.ascontiguousarray(out_offsets, dtype=np.int64),
            "poly_edges": plan.edges, "poly_sizes": plan.hw.astype(np.int32), "poly_blocks": _blocks(plan.hw)}


def _sorted_positions(t, plan, device):
    """The crossings kernel and the one sort -> device int32 positions, polygon after polygon."""
    keys = torch.empty(max(plan.total, 1), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _native.call("m2f_poly_crossings", _native.ptr_or_null(t["poly_edges"]), _native.ptr_or_null(t["poly_slopes"]),
                     _native.ptr_or_null(t["poly_starts"]), plan.edges.shape[0], plan.total, keys.data_ptr(),
                     _native.stream(device))
    keys = torch.sort(keys[:plan.total])[0]
    return (keys & 0x7fffffff).to(torch.int32)


def _launch_polygons(t, plan, words, device):
    """Crossings, sort and decode of the planned annotations into ``words`` at ``poly_out_offsets``."""
    if plan.num_anns == 0:
        return
    pos = _sorted_positions(t, plan, device)
    with torch.cuda.device(device):
        _native.call("m2f_poly_decode_bits_ragged", _native.ptr_or_null(pos), pos.numel(),
                     t["poly_pos_offsets"].data_ptr(), plan.num_polys, t["poly_part_offsets"].data_ptr(), plan.num_anns,
                     t["poly_sizes"].data_ptr(), t["poly_out_offsets"].data_ptr(),
                     _native.ptr_or_null(t["poly_blocks"]), t["poly_blocks"].numel() // 2, _native.ptr_or_null(words),
                     words.numel(), _native.stream(device))


def _rasterize(plan, out_offsets, total_words, device):
    if device.type != "cuda":
        return torch.from_numpy(_decode_host(_crossings_host(plan), plan, out_offsets, total_words)).to(device)
    dev = _native.upload_tables(_tables(plan, out_offsets), device)   # one copy
    words = torch.empty(total_words, dtype=torch.int32, device=device)
    _launch_polygons(dev, plan, words, device)
    return words


# -------------------------------------------------------------------------------------------------------------------
# public: positions, planes
# -------------------------------------------------------------------------------------------------------------------
def polygon_crossings(polys, sizes, device=None):
    """polys: a list of polygons, each a flat ``[x0, y0, x1, y1, ...]``; sizes: one ``(H, W)`` for all or one per
    polygon.  -> ``(positions, offsets)``: ``positions`` a flat int32 tensor on ``device``, polygon ``i`` owning the
    sorted ``positions[offsets[i]:offsets[i + 1]]`` (its kept crossings and, last, the sentinel ``H W``);
    ``offsets`` a host int64 array.  The offsets follow from the vertices alone (rule 3), before anything runs.

    Raises ValueError, before any launch, on what :func:`check_annotation` refuses and when ``H W >= 2^31``."""
    device = torch.device("cpu" if device is None else device)
    polys = list(polys)
    hw = _sizes(sizes, len(polys), "polygons")
    plan = _plan([[p] for p in polys], hw, [f"polygon {i}" for i in range(len(polys))])
    if device.type != "cuda":
        return torch.from_numpy(_crossings_host(plan)).to(device), plan.pos_offsets
    if plan.total == 0:
        return torch.zeros(0, dtype=torch.int32, device=device), plan.pos_offsets
    dev = _native.upload_tables(_tables(plan, np.zeros(plan.num_anns, np.int64)), device)
    return _sorted_positions(dev, plan, device), plan.pos_offsets


def polygons_to_bits_ragged(anns, sizes, device=None, names=None):
    """anns[m]: the polygons of annotation ``m`` (a list of flat coordinate lists; ``[]`` is a zero mask);
    ``sizes[m] = (H, W)``.  -> ``(words, offsets, sizes)`` exactly as :func:`~bm2f_amd.mask_iou.rle_to_bits_ragged`
    returns them: planes of ``H_m * ceil(W_m / 32)`` words on multiples of 4 words, tail bits zero, padding words
    unspecified on the device.  On a HIP device: one upload, the crossings kernel, one sort and the decode kernel,
    whatever the number of annotations, parts and sizes.  ``names[m]`` is what an error calls annotation ``m``.

    Raises ValueError, before any launch, on what :func:`check_annotation` refuses, when ``H W >= 2^31`` and when
    the planes take more than ``MAX_RAGGED_WORDS`` words."""
    device = torch.device("cpu" if device is None else device)
    anns = list(anns)
    if not anns:
        return torch.zeros(0, dtype=torch.int32, device=device), np.zeros(0, np.int64), np.zeros((0, 2), np.int64)
    hw = _sizes(sizes, len(anns), "annotations")
    plan = _plan(anns, hw, names)
    padded = (_plane_words(hw) + _PLANE_ALIGN - 1) // _PLANE_ALIGN * _PLANE_ALIGN
    out_offsets = np.concatenate(([0], np.cumsum(padded)))[:-1].astype(np.int64)
    total = int(padded.sum())
    if total > MAX_RAGGED_WORDS:
        raise ValueError(f"the planes take {total} words, more than the {MAX_RAGGED_WORDS} of one buffer; "
                         "split the annotations over several calls")
    return _rasterize(plan, out_offsets, total, device), out_offsets, hw


def polygons_to_bits(anns, size, device=None, names=None) -> torch.Tensor:
    """Annotations of one image size -> (M, H, ceil(W / 32)) int32 planes on ``device``, the layout of
    :func:`~bm2f_amd.mask_iou.rle_to_bits` (what ``mask_pair_counts`` and the clip targets take)."""
    device = torch.device("cpu" if device is None else device)
    anns = list(anns)
    H, W = int(size[0]), int(size[1])
    _check_size(H, W)
    n = H * ((W + 31) // 32)
    if not anns:
        return torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=device)
    if len(anns) * n > MAX_RAGGED_WORDS:
        raise ValueError(f"the planes take {len(anns) * n} words, more than the {MAX_RAGGED_WORDS} of one call")
    plan = _plan(anns, _sizes((H, W), len(anns), "annotations"), names)
    words = _rasterize(plan, np.arange(len(anns), dtype=np.int64) * n, len(anns) * n, device)
    return words.view(len(anns), H, -1)


# -------------------------------------------------------------------------------------------------------------------
# public: RLE
# -------------------------------------------------------------------------------------------------------------------
def polygons_to_rle(polys, h, w, device=None) -> list:
    """``pycocotools.mask.frPyObjects`` on a list of polygons: one canonical RLE dict per polygon, rasterised and
    encoded (``rle_encode`` on the packed bits) on ``device``."""
    polys = list(polys)
    if not polys:
        _check_size(int(h), int(w))
        return []
    names = [f"polygon {i}" for i in range(len(polys))]
    return rle_encode(polygons_to_bits([[p] for p in polys], (h, w), device, names), width=int(w))


def ann_to_rle(segmentation, h, w, device=None) -> dict:
    """``COCO.annToRLE``: a polygon list is rasterised and united into one RLE, an uncompressed RLE (``counts`` a
    list) is compressed as it stands, a compressed RLE is returned as it is."""
    h, w = int(h), int(w)
    if isinstance(segmentation, dict):
        if [int(v) for v in segmentation["size"]] != [h, w]:
            raise ValueError(f"the RLE has size {list(segmentation['size'])}, {[h, w]} was expected")
        counts = segmentation["counts"]
        if isinstance(counts, (str, bytes)):
            return segmentation
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
        if (c < 0).any() or int(c.sum()) != h * w:
            raise ValueError("counts do not add up to the mask size")
        return {"size": [h, w], "counts": counts_to_string(c.tolist())}
    return rle_encode(polygons_to_bits([segmentation], (h, w), device), width=w)[0]


def convert_polygons_to_rle(dataset, device=None, batch_bytes=DEFAULT_BATCH_BYTES) -> dict:
    """A copy of a COCO instances dict with every polygon segmentation replaced by its RLE (everything else,
    ``area`` included, is kept): the file ``COCOGroundTruth`` reads with its default ``polygons="refuse"``.  The
    annotations are rasterised and encoded on ``device`` in batches of one image size and at most ``batch_bytes``
    of planes, so the number of launches grows with the number of distinct sizes and batches, not of annotations."""
    device = torch.device("cpu" if device is None else device)
    out = copy.copy(dataset)
    out["annotations"] = [dict(a) for a in dataset.get("annotations", [])]
    imgs = {im["id"]: im for im in dataset.get("images", [])}
    by_size = {}
    for i, ann in enumerate(out["annotations"]):
        seg = ann.get("segmentation")
        if seg is None or isinstance(seg, dict):
            continue
        if ann["image_id"] not in imgs:
            raise ValueError(f"annotation {ann.get('id')} names an image the dataset does not hold")
        img = imgs[ann["image_id"]]
        by_size.setdefault((int(img["height"]), int(img["width"])), []).append(i)
    todo = []
    for (H, W), members in by_size.items():                          # every check before the first launch
        _check_size(H, W)
        names = [f"annotation {out['annotations'][i].get('id')}" for i in members]
        for i, name in zip(members, names):
            check_annotation(out["annotations"][i]["segmentation"], name)
        per = max(1, int(batch_bytes) // (4 * H * ((W + 31) // 32)))
        todo += [((H, W), members[a:a + per], names[a:a + per]) for a in range(0, len(members), per)]
    for (H, W), members, names in todo:
        bits = polygons_to_bits([out["annotations"][i]["segmentation"] for i in members], (H, W), device, names)
        for i, rle in zip(members, rle_encode(bits, width=W)):
            out["annotations"][i]["segmentation"] = rle
    return out


# -------------------------------------------------------------------------------------------------------------------
# the evaluator's batch step with polygon ground truth
# -------------------------------------------------------------------------------------------------------------------
def is_polygon(segmentation) -> bool:
    return isinstance(segmentation, (list, tuple))


def pair_counts_ragged(masks, groups, device=None, sizes=None, names=None):
    """:func:`~bm2f_amd.mask_iou.rle_pair_counts_ragged` for a batch in which a mask is an RLE dict, ``None`` or a
    polygon annotation (a list of polygons, whose (H, W) ``sizes[m]`` gives): the RLE masks and the polygon
    annotations are written into one ragged buffer, by the RLE decoder and by the polygon kernels, and counted
    together.  On a HIP device: one upload, a number of launches that does not depend on the batch (the RLE
    decoder, the crossings kernel, one sort, the polygon decoder, the two pair-count kernels) and one copy.  A batch
    without polygons is handed to ``rle_pair_counts_ragged`` as it is."""
    masks = list(masks)
    poly = np.array([is_polygon(m) for m in masks], dtype=bool)
    if not poly.any():
        return rle_pair_counts_ragged(masks, groups, device=device, sizes=sizes)
    device = torch.device("cpu" if device is None else device)
    groups = list(groups)
    if not groups:
        return []
    rles = [None if p else m for m, p in zip(masks, poly)]
    hw, out_offsets, total, dtables = _decode_plan(rles, sizes)
    dtables["blocks"] = dtables["blocks"][~poly[dtables["blocks"][:, 0]]]     # the RLE decoder skips polygon planes
    which = np.flatnonzero(poly)
    plan = _plan([masks[i] for i in which], hw[which], None if names is None else [names[i] for i in which])
    desc, ptables, num_tiles = _pair_plan(_groups_by_offset(groups, hw, out_offsets), total)
    if device.type != "cuda":
        words = rle_to_bits_ragged(rles, device, sizes)[0].numpy()    # zero planes where the polygons go
        words = words | _decode_host(_crossings_host(plan), plan, out_offsets[which], total)
        return _pair_counts_ragged_host(words, desc, ptables)
    dev = _native.upload_tables({**dtables, **_tables(plan, out_offsets[which]), **ptables}, device)
    words = torch.empty(total, dtype=torch.int32, device=device)
    _launch_decode(dev, len(rles), words, device)
    _launch_polygons(dev, plan, words, device)
    out = _launch_pairs(words, desc, dev, num_tiles, device)
    return _split_counts(out.cpu().numpy(), desc)                     # the one copy
