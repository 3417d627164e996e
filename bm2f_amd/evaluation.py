"""Result writers: the head outputs as the JSON-serialisable lists the reference's evaluators dump
(``instances_to_coco_json_video``, mask2former_video/data_video/ytvis_eval.py:256-293, and the COCO instance
results detectron2 writes for mask2former/evaluation/instance_evaluation.py).  Masks go out as COCO RLE
(``bm2f_amd.rle``); outputs the heads already encoded (``rle=True`` / ``instance_rle=True``) pass through, bool,
float and packed masks are encoded here with :func:`rle_encode`.  The video metrics are computed in
``bm2f_amd.ytvis_eval``."""
from __future__ import annotations

import torch

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
