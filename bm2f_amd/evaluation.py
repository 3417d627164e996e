"""Result writers: the head outputs as the JSON-serialisable lists the reference's evaluators dump
(``instances_to_coco_json_video``, mask2former_video/data_video/ytvis_eval.py:256-293, and the COCO instance
results detectron2 writes for mask2former/evaluation/instance_evaluation.py).  Masks go out as COCO RLE
(``bm2f_amd.rle``); outputs the heads already encoded (``rle=True`` / ``instance_rle=True``) pass through, bool,
float and packed masks are encoded here with :func:`rle_encode`.  The video metrics are computed in
``bm2f_amd.ytvis_eval``.

Label maps go out through ``bm2f_amd.label_rle``: detectron2's ``sem_seg_predictions.json``
(:func:`sem_seg_to_coco_json`, read back by :func:`load_sem_seg_predictions`), COCO annotations of a panoptic id map
(:func:`panoptic_to_coco_detection`) and of an ADE20K instance map (:func:`instance_map_annotations`)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .label_planes import as_label_plane, same_dtype
from .label_rle import label_maps_to_rle, rle_to_label_maps
from .rle import rle_encode


def _as_list(v):
    return v.tolist() if torch.is_tensor(v) else list(v)


def _plain(rle):
    counts = rle["counts"]
    return {"size": [int(s) for s in rle["size"]],
            "counts": counts.decode("ascii") if isinstance(counts, bytes) else str(counts)}


def instances_to_coco_json_video(inputs, outputs):
    """inputs: the one-video batch ``[{"video_id": ..., ...}]``; outputs: the dict of
    :class:`VideoMaskFormerInference` (bool, ``packed=True`` or ``rle=True`` masks).  -> one
    ``{"video_id", "score", "category_id", "segmentations"}`` per predicted instance, ``segmentations`` holding one
    RLE per frame (ytvis_eval.py:256-293)."""
    assert len(inputs) == 1, "More than one inputs are loaded for inference!"
    video_id = inputs[0]["video_id"]
    scores, labels, masks = outputs["pred_scores"], outputs["pred_labels"], outputs["pred_masks"]
    width = outputs["image_size"][1]
    results = []
    for s, l, m in zip(_as_list(scores), _as_list(labels), masks):
        if outputs.get("rle"):
            segms = m
        elif outputs.get("packed"):
            segms = rle_encode(m, width=width)
        else:
            segms = rle_encode(m.bool() if torch.is_tensor(m) else torch.as_tensor(m).bool())
        results.append({"video_id": video_id, "score": float(s), "category_id": int(l),
                        "segmentations": [_plain(r) for r in segms]})
    return results


def instances_to_coco_json(instances, img_id):
    """instances: the ``"instances"`` dict of :class:`MaskFormerInference` (``pred_masks_rle`` or float / bool
    ``pred_masks``).  -> one ``{"image_id", "category_id", "bbox", "score", "segmentation"}`` per instance, ``bbox``
    being ``pred_boxes`` (XYXY) as XYWH."""
    scores, classes = _as_list(instances["scores"]), _as_list(instances["pred_classes"])
    if len(scores) == 0:
        return []
    boxes = torch.as_tensor(instances["pred_boxes"]).detach().float().cpu().clone()
    boxes[:, 2:] -= boxes[:, :2]
    if "pred_masks_rle" in instances:
        rles = instances["pred_masks_rle"]
    else:
        m = instances["pred_masks"]
        rles = rle_encode(m if m.dtype in (torch.bool, torch.uint8) else m > 0)
    return [{"image_id": img_id, "category_id": int(c), "bbox": [float(v) for v in b], "score": float(s),
             "segmentation": _plain(r)}
            for s, c, b, r in zip(scores, classes, boxes.tolist(), rles)]


# -------------------------------------------------------------------------------------------------------------------
# label maps: semantic result files, panoptic and instance-map annotations (bm2f_amd.label_rle)
# -------------------------------------------------------------------------------------------------------------------
def _label_batch(maps):
    """Integer label maps (tensors or arrays, any integer dtype) -> tensors of one of uint8 / int16 / int32."""
    planes = [as_label_plane(m, f"label map {k}") for k, m in enumerate(maps)]
    return same_dtype([m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)) for m in planes])


def sem_seg_to_coco_json(label_maps, file_names, *, contiguous_id_to_dataset_id=None, ignore=None):
    """label_maps: one (H, W) integer label map per image (the ``sem_seg.argmax(0)`` of detectron2's
    ``SemSegEvaluator.process``); file_names: their ``file_name``.  -> detectron2's ``sem_seg_predictions.json`` list
    (``encode_json_sem_seg``): one ``{"file_name", "category_id", "segmentation": {"size", "counts"}}`` per class
    present per image, classes ascending, from one :func:`label_maps_to_rle` call.  With a mapping ``category_id`` is
    the dataset id and a label absent from it raises ValueError (detectron2 asserts there); without one it is
    ``int(label)``.  Pixels equal to ``ignore`` are written under no class."""
    label_maps, file_names = list(label_maps), list(file_names)
    if len(label_maps) != len(file_names):
        raise ValueError(f"{len(label_maps)} label maps and {len(file_names)} file names")
    results = []
    for name, segments in zip(file_names, label_maps_to_rle(_label_batch(label_maps), ignore=ignore)):
        for seg in segments:
            label = seg["label"]
            if contiguous_id_to_dataset_id is None:
                category_id = int(label)
            elif label in contiguous_id_to_dataset_id:
                category_id = int(contiguous_id_to_dataset_id[label])
            else:
                raise ValueError(f"{name}: the label {label} is not in contiguous_id_to_dataset_id")
            results.append({"file_name": name, "category_id": category_id, "segmentation": seg["segmentation"]})
    return results


def sem_seg_image_id(file_name):
    """The image id the reference's tools/evaluate_pq_for_semantic_segmentation.py takes from a ``file_name``."""
    return os.path.basename(file_name).split(".")[0]


def load_sem_seg_predictions(json_or_list, sizes, *, dataset_id_to_contiguous_id=None, device=None):
    """json_or_list: the path of a ``sem_seg_predictions.json`` or its list; sizes: ``{image_id: (H, W)}`` with
    ``image_id = os.path.basename(file_name).split(".")[0]``.  -> ``{image_id: (H, W) int32 label map on device}`` for
    every image of ``sizes``: zeros painted with ``category_id`` (mapped through ``dataset_id_to_contiguous_id`` when
    given; a category absent from it raises ValueError) in file order, as the reference tool does, by one
    :func:`rle_to_label_maps` call.  An entry whose image is not in ``sizes`` raises ValueError."""
    if isinstance(json_or_list, (str, os.PathLike)):
        with open(json_or_list) as f:
            json_or_list = json.load(f)
    ids = list(sizes)
    per_image = {i: [] for i in ids}
    for entry in json_or_list:
        image_id = sem_seg_image_id(entry["file_name"])
        if image_id not in per_image:
            raise ValueError(f"{entry['file_name']}: no size is given for the image {image_id!r}")
        category_id = entry["category_id"]
        if dataset_id_to_contiguous_id is not None:
            if category_id not in dataset_id_to_contiguous_id:
                raise ValueError(f"{entry['file_name']}: the category {category_id} is not in "
                                 "dataset_id_to_contiguous_id")
            category_id = dataset_id_to_contiguous_id[category_id]
        per_image[image_id].append((int(category_id), entry["segmentation"]))
    planes = rle_to_label_maps([per_image[i] for i in ids], [sizes[i] for i in ids], fill=0, dtype=torch.int32,
                               device=device)
    return dict(zip(ids, planes))


def _is_thing(categories, category_id):
    if categories is None:
        raise ValueError("things_only needs the categories")
    if not isinstance(categories, dict):
        categories = {c["id"]: c for c in categories}
    return categories[category_id]["isthing"] == 1


def panoptic_to_coco_detection(image_id, id_map, segments_info, *, first_id=1, things_only=False, categories=None):
    """id_map: the (H, W) segment-id map of a panoptic PNG (``rgb2id``); segments_info: its ``{"id", "category_id",
    ["iscrowd"]}`` dicts.  -> one ``{"id", "image_id", "category_id", "iscrowd", "bbox", "area", "segmentation"}`` per
    segment in ``segments_info`` order (with ``things_only`` those whose category has ``isthing == 1`` in
    ``categories``), ``id`` counting from ``first_id``: the role of panopticapi's panoptic-to-detection converter.
    ``segmentation`` is the RLE of ``id_map == id``; ``bbox`` ``[xmin, ymin, w, h]`` and ``area`` are taken from the
    map itself (a segment without pixels: the all-zero RLE, zeros)."""
    keep = [s for s in segments_info if not things_only or _is_thing(categories, s["category_id"])]
    plane, = _label_batch([id_map])
    entries, = label_maps_to_rle([plane], ids=[[int(s["id"]) for s in keep]])
    return [{"id": first_id + k, "image_id": image_id, "category_id": int(s["category_id"]),
             "iscrowd": int(s.get("iscrowd", 0)), "bbox": e["bbox"], "area": e["area"],
             "segmentation": e["segmentation"]} for k, (s, e) in enumerate(zip(keep, entries))]


def instance_map_annotations(ids_plane, cats_plane, image_id, *, cat_map=None, first_id=1):
    """ids_plane, cats_plane: the (H, W) uint8 instance-id and category planes of an ADE20K instance PNG; instance id
    0 is VOID.  -> one ``{"id", "image_id", "iscrowd": 0, "category_id", "bbox", "segmentation", "area"}`` per
    instance id in ascending order, ``category_id = cat_map[category]`` when a mapping is given: the per-image body
    of the reference's datasets/prepare_ade20k_ins_seg.py.  One :func:`label_maps_to_rle` call on the combined plane
    ``category * 256 + id``; an instance under more than one category raises ValueError (the script asserts)."""
    ids_plane, cats_plane = _label_batch([ids_plane])[0], _label_batch([cats_plane])[0]
    if ids_plane.dtype != torch.uint8 or cats_plane.dtype != torch.uint8:
        raise ValueError("the instance-id and category planes must be uint8")
    if ids_plane.shape != cats_plane.shape or ids_plane.device != cats_plane.device:
        raise ValueError("the two planes must share their shape and device")
    combined = cats_plane.to(torch.int32) * 256 + ids_plane.to(torch.int32)
    entries, = label_maps_to_rle([combined])
    by_id = {}
    for e in entries:
        category, instance = divmod(e["label"], 256)
        if instance == 0:
            continue
        if instance in by_id:
            raise ValueError(f"image {image_id}: the instance {instance} lies under the categories "
                             f"{by_id[instance][0]} and {category}")
        by_id[instance] = (category, e)
    out = []
    for k, instance in enumerate(sorted(by_id)):
        category, e = by_id[instance]
        out.append({"id": first_id + k, "image_id": image_id, "iscrowd": 0,
                    "category_id": int(cat_map[category]) if cat_map is not None else int(category),
                    "bbox": e["bbox"], "segmentation": e["segmentation"], "area": e["area"]})
    return out
