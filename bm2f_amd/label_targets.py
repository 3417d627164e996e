"""Training targets of semantic and panoptic datasets as they ship: one label map per image, not one mask per segment.

A *label-map target* is a dict

    ``"labels"``     (G,) int64 class of every target, as in a dense target;
    ``"label_map"``  (H, W) integer map (uint8, int16, int32; int64 is converted to int32 where it is consumed);
    ``"ids"``        (G,) integer ids (int32 on a device);

target ``g`` being the set ``label_map == ids[g]``.  It is equivalent to the dense target ``{"labels", "masks":
label_map[None] == ids[:, None, None]}`` (:func:`label_targets_to_masks`), and the mask-supervised matcher and
criterion (``bm2f_amd/mask_criterion.py``) accept it in place of one: on a HIP device they read the map and the ids in
place (``m2f_point_match_cost_labels``, ``m2f_point_loss_fwd_labels`` / ``_bwd_labels`` in ``csrc/point_sample.hip``),
bitwise as they would read the dense planes, which then never exist.  A pixel whose label is no id (the ignore label,
VOID, a crowd segment) belongs to no target.

The two helpers restate what the reference's dataset mappers do between the decoded annotation and ``prepare_targets``:

:func:`semantic_targets`   ``MaskFormerSemanticDatasetMapper``: ``classes = np.unique(sem_seg)`` without the ignore
                           label, ``masks = [sem_seg == c for c in classes]``.
:func:`panoptic_targets`   ``MaskFormerPanopticDatasetMapper`` / ``COCOPanopticNewBaselineDatasetMapper``: one mask
                           ``pan_seg == s["id"]`` per non-crowd entry of ``segments_info``.

Reading files, ``rgb2id`` (``bm2f_amd.rgb2id``) and the mappers' augmentations stay with the caller.  Panoptic ids are
``r + 256 g + 256^2 b < 2^24``; any id that fits an int32 works.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native
from .label_counts import label_histogram_ragged
from .label_planes import as_label_maps                     # mask_criterion imports it from here


def _device_of(maps):
    devices = {m.device for m in maps if m.device.type == "cuda"}
    if len(devices) > 1:
        raise ValueError(f"maps on several devices: {sorted(map(str, devices))}")
    return devices.pop() if devices else torch.device("cpu")


def _id_tables(per_image, device):
    """per_image: a list of dicts of equally long host int64 arrays, ``"ids"`` among them -> the same as tensors on
    ``device`` (ids int32, the rest int64), the whole batch in one copy."""
    names = list(per_image[0]) if per_image else []
    flat = {k: np.concatenate([p[k] for p in per_image]).astype(np.int32 if k == "ids" else np.int64) for k in names}
    if device.type == "cuda":
        dev = _native.upload_tables(flat, device)                                                # one copy
    else:
        dev = {k: torch.from_numpy(v) for k, v in flat.items()}
    out, at = [], 0
    for p in per_image:
        n = p["ids"].size
        out.append({k: dev[k][at:at + n] for k in names})
        at += n
    return out


def semantic_targets(sem_segs, ignore_label, num_classes):
    """sem_segs: a list of (H_b, W_b) semantic label maps of any sizes (integer tensors or arrays; int64 is converted
    to int32 once).  -> one label-map target per image: ``ids = labels =`` the classes present in the map other than
    ``ignore_label``, ascending (``np.unique``'s order), and ``"areas"`` (G,) int64, their pixel counts.  An image of
    ignored pixels alone has G = 0.  A value outside ``[0, num_classes)`` that is not ``ignore_label`` raises
    ValueError naming the image.

    With maps on a HIP device the present classes of the whole batch come from one launch of the label histogram
    (:func:`bm2f_amd.label_histogram_ragged`) and one copy to the host; the id tables go back in one copy.  On CPU
    tensors the same definition runs in numpy."""
    maps = as_label_maps(sem_segs, "sem_seg")
    if not maps:
        return []
    device = _device_of(maps)
    num_classes = int(num_classes)
    ignore = None if ignore_label is None else int(ignore_label)
    counts, bad = label_histogram_ragged(maps, num_classes, ignore)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"sem_seg of image {b}: {int(bad[b])} pixels are neither in [0, {num_classes}) nor the "
                         f"ignore label {ignore_label}")
    per_image = []
    for b in range(len(maps)):
        hist = counts[b, :num_classes]
        if ignore is not None and 0 <= ignore < num_classes:
            hist = hist.copy()
            hist[ignore] = 0                        # counted in the last column; an ignored class is no target
        present = np.flatnonzero(hist).astype(np.int64)
        per_image.append({"labels": present, "ids": present, "areas": hist[present].astype(np.int64)})
    tables = _id_tables(per_image, device)
    return [dict(t, label_map=m.to(device)) for t, m in zip(tables, maps)]


def panoptic_targets(pan_segs, segments_infos):
    """pan_segs: a list of (H_b, W_b) panoptic id maps (after ``rgb2id``; ids below 2^24, int64 is converted to int32
    once); segments_infos: per image the list of dicts with ``id``, ``category_id`` and ``iscrowd``.  -> one label-map
    target per image: ``ids`` the ids and ``labels`` the category ids of the non-crowd segments, in list order.  A
    listed segment without pixels is kept, as the reference keeps it: its target is empty.

    Everything is known on the host: nothing synchronises with the device, and the id tables of the batch go up in
    one copy."""
    maps = as_label_maps(pan_segs, "pan_seg")
    if len(segments_infos) != len(maps):
        raise ValueError(f"{len(maps)} maps and {len(segments_infos)} segment lists")
    if not maps:
        return []
    device = _device_of(maps)
    per_image = []
    for b, infos in enumerate(segments_infos):
        kept = [s for s in infos if not s.get("iscrowd", 0)]
        ids = np.array([int(s["id"]) for s in kept], dtype=np.int64)
        if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise ValueError(f"segments_info of image {b}: ids must fit an int32")
        per_image.append({"labels": np.array([int(s["category_id"]) for s in kept], dtype=np.int64), "ids": ids})
    tables = _id_tables(per_image, device)
    return [dict(t, label_map=m.to(device)) for t, m in zip(tables, maps)]


def label_targets_to_masks(target):
    """The dense equivalent of a label-map target: (G, H, W) bool, ``label_map == ids[g]`` (plain torch)."""
    m, ids = target["label_map"], target["ids"]
    if m.dim() != 2 or ids.dim() != 1:
        raise ValueError("label_map must be (H, W) and ids (G,)")
    return m[None].to(torch.int64) == ids.to(m.device)[:, None, None].to(torch.int64)
