"""Video instance AP: the reference's ``YTVISEvaluator.evaluate()`` (mask2former_video/data_video/ytvis_eval.py:115-253)
and what it drives, ``YTVOS`` (data_video/datasets/ytvis_api/ytvos.py) and ``YTVOSeval`` (ytvis_api/ytvoseval.py),
restated without pycocotools and detectron2.  ``file:line`` below are lines of ytvoseval.py unless a file is named.

The mask work (the reference's ``computeIoU``, :176-222: one ``pycocotools.mask.merge`` and ``area`` per detection,
ground truth and frame) runs on bit planes: per video, every ground-truth frame and every detection frame becomes a
plane (``rle_to_bits``, or the head's ``pred_bits``), one ``mask_pair_counts`` launch counts all pairs of the video
over all categories, and the host slices by category.  A missing frame (``None``) is a zero plane on either side, which
is what the three branches of ``iou_seq`` (:203-217) add up to: ``i = sum |d & g|``, ``u = sum |d| + sum |g| - i``.

Matching, accumulation and the summary are those of ``bm2f_amd.ap_eval``, on the host in numpy, vectorised over the
IoU thresholds; they handle at most ``maxDets[-1]`` detections times a handful of objects per (video, category) and
are not the hot path.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from .ap_eval import VIDEO, APEvaluator, EvalResult, evaluate_units, normalize_params
from .evaluation import instances_to_coco_json_video
from .mask_iou import mask_pair_counts, rle_to_bits


class YTVISParams:
    """The evaluation parameters (``Params.setDetParams``, :534-545)."""

    def __init__(self):
        self.vidIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = 'segm'


def _avg_area(areas):
    """``l = [a for a in ann['areas'] if a]``; the mean, 0 when empty (:100-104 and ytvos.py:250-254)."""
    kept = [a for a in areas if a]
    return 0 if len(kept) == 0 else np.array(kept).mean()


class YTVISGroundTruth:
    """A YTVIS annotation file (or the dict it holds): videos, categories and annotations indexed as ``YTVOS``
    (ytvos.py:68-97) does.  ``avg_area`` of an annotation is the mean over the truthy entries of its ``areas``, 0 if
    there are none (``_toMask``, :100-104).  Segmentations are RLE (compressed or uncompressed) or ``None``; polygons
    raise NotImplementedError."""

    def __init__(self, dataset):
        if isinstance(dataset, (str, bytes)) or hasattr(dataset, "__fspath__"):
            with open(dataset) as f:
                dataset = json.load(f)
        if not isinstance(dataset, dict):
            raise ValueError("the ground truth must be a dict or the path of a JSON file holding one")
        self.dataset = dataset
        self.videos = {v["id"]: v for v in dataset.get("videos", [])}
        self.cats = {c["id"]: c for c in dataset.get("categories", [])}
        self.anns = list(dataset.get("annotations", []))
        self.has_annotations = "annotations" in dataset
        self.vid_to_anns = {}
        for ann in self.anns:
            for seg in ann["segmentations"]:
                if seg and not isinstance(seg, dict):
                    raise NotImplementedError("polygon segmentations are not supported: YTVIS ships RLE")
            self.vid_to_anns.setdefault(ann["video_id"], []).append(ann)

    def video_ids(self):
        return list(self.videos.keys())

    def category_ids(self):
        return [c["id"] for c in self.dataset.get("categories", [])]


class YTVISEvalResult(EvalResult):
    """What ``YTVOSeval`` holds after ``evaluate()``, ``accumulate()`` and ``summarize()``."""


# -------------------------------------------------------------------------------------------------------------------
# device part: the counts of one video
# -------------------------------------------------------------------------------------------------------------------
def _frames(anns, what):
    lengths = {len(a["segmentations"]) for a in anns}
    if len(lengths) > 1:
        raise ValueError(f"{what}: sequences of different lengths {sorted(lengths)} in one video")
    return lengths.pop() if lengths else 0


def video_pair_counts(gt, video_id, dets, device=None, pred_bits=None):
    """All detections of one video against all of its ground truths, over all categories, in one launch:
    -> (inter (D, G), area_d (D, T), area_g (G, T)) host int64, G in the order of ``gt.vid_to_anns[video_id]``.
    ``pred_bits`` (D, T, H, words), when given, stands for the detections' segmentations."""
    device = torch.device("cpu" if device is None else device)
    vid = gt.videos[video_id]
    H, W = int(vid["height"]), int(vid["width"])
    gts = gt.vid_to_anns.get(video_id, [])
    Tg = _frames(gts, "ground truth")
    if pred_bits is not None:
        D, Td = int(pred_bits.shape[0]), int(pred_bits.shape[1])
        if D != len(dets) or tuple(pred_bits.shape[2:]) != (H, (W + 31) // 32):
            raise ValueError(f"pred_bits {tuple(pred_bits.shape)} do not fit {len(dets)} detections of {H} x {W}")
    else:
        D, Td = len(dets), _frames(dets, "detections")
    G = len(gts)
    T = Td if D else Tg
    if D and G and Td != Tg:
        raise ValueError(f"video {video_id}: detections of {Td} frames, ground truth of {Tg}")
    words = (W + 31) // 32
    rles = [] if pred_bits is not None else [s if s else None for d in dets for s in d["segmentations"]]
    n_d = len(rles)
    rles += [s if s else None for g in gts for s in g["segmentations"]]
    planes = rle_to_bits(rles, device=device, size=(H, W))            # one parse, one upload, one launch
    a = pred_bits.to(device) if pred_bits is not None else planes[:n_d].view(D, T, H, words)
    b = planes[n_d:].view(G, T, H, words)
    return mask_pair_counts(a, b, W)


def evaluate_ytvis(gt, results, device=None, params=None, pred_bits=None, _counts=None) -> YTVISEvalResult:
    """gt: a :class:`YTVISGroundTruth`; results: the list ``instances_to_coco_json_video`` writes (``video_id``,
    ``score``, ``category_id``, ``segmentations`` with one RLE or ``None`` per frame); ``pred_bits`` optionally maps
    a video id to the (D, T, H, words) planes of that video's results, in their order, which are then not decoded.
    ``device`` is where the planes are built and counted (CPU by default).  Only ``iouType="segm"`` and
    ``useCats=1`` are supported.

    The rules (ordering, the ``maxDets[-1]`` cut per (video, category), matching thresholds and ties, the crowd
    re-match, the break on ignore, float32 accumulation, the -1 conventions, the 12 statistics) are listed in
    ``bm2f_amd.ap_eval``.  Sequences of one video must have one length (the reference's ``zip`` would cut them to the
    shorter)."""
    src = params if params is not None else YTVISParams()
    if getattr(src, "iouType", "segm") != "segm" or getattr(src, "useSegm", None) is not None:
        raise NotImplementedError("only iouType='segm' is supported")
    p = normalize_params(VIDEO, src, gt.video_ids(), gt.category_ids(), results,
                         "results name videos the ground truth does not hold")      # ytvos.py:231
    if any("segmentations" not in r for r in results):
        raise ValueError("results must hold 'segmentations'")

    def counts_of(vidId, anns, dets):
        if _counts is not None and vidId in _counts:
            return _counts[vidId]
        return video_pair_counts(gt, vidId, dets, device, pred_bits.get(vidId) if pred_bits else None)

    def dt_area(r, areas):
        return _avg_area([int(a) if s else None for a, s in zip(areas, r["segmentations"])])

    return evaluate_units(p, VIDEO, gt.vid_to_anns, results, counts_of, lambda ann: _avg_area(ann["areas"]), dt_area,
                          crowd_iou=False, result_cls=YTVISEvalResult)


# -------------------------------------------------------------------------------------------------------------------
# the evaluator
# -------------------------------------------------------------------------------------------------------------------
class YTVISEvaluator(APEvaluator):
    """The reference's ``YTVISEvaluator`` (ytvis_eval.py:27-253) without detectron2: ``reset()``, ``process(inputs,
    outputs)`` per video and ``evaluate()``.

    ``process`` takes the dict of :class:`VideoMaskFormerInference` in any of its forms (bool, ``packed=True``,
    ``rle=True``).  When it holds ``"pred_bits"`` (``keep_bits=True``) the video's pair counts are taken at once from
    those planes, on their device, and only the counts are kept: the predictions are neither uploaded nor decoded
    again.  ``results`` is the accumulated ``results.json`` list (contiguous category ids, as the head wrote them)."""

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id=None, class_names=None, device=None,
                 params=None):
        gt = ground_truth if isinstance(ground_truth, YTVISGroundTruth) else YTVISGroundTruth(ground_truth)
        super().__init__(gt, thing_dataset_id_to_contiguous_id, class_names, device, params)

    def reset(self):
        super().reset()
        self._counts = {}

    def process(self, inputs, outputs):
        prediction = instances_to_coco_json_video(inputs, outputs)
        self._predictions.extend(prediction)
        bits = outputs.get("pred_bits")
        if bits is not None and len(prediction) and self.gt.has_annotations:
            video_id = inputs[0]["video_id"]
            if video_id in self._counts:
                raise ValueError(f"video {video_id} was processed twice")
            device = bits.device if self.device is None else self.device
            self._counts[video_id] = video_pair_counts(self.gt, video_id, prediction, device, bits)

    def _mapped(self):
        """The predictions with dataset category ids (ytvis_eval.py:152-166)."""
        predictions = [dict(r) for r in self._predictions]
        if self.id_map is not None:
            all_contiguous_ids = list(self.id_map.values())
            num_classes = len(all_contiguous_ids)
            assert min(all_contiguous_ids) == 0 and max(all_contiguous_ids) == num_classes - 1
            reverse = {v: k for k, v in self.id_map.items()}
            for r in predictions:
                assert r["category_id"] < num_classes, (
                    f"A prediction has class={r['category_id']}, but the dataset only has {num_classes} classes")
                r["category_id"] = reverse[r["category_id"]]
        return predictions

    def evaluate(self):
        """-> ``{"segm": {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AP-<name>", ...}}`` in percent,
        NaN where the reference's summary is negative (``_derive_coco_results``, ytvis_eval.py:193-253); ``{}`` without
        predictions or without annotations."""
        if len(self._predictions) == 0 or not self.gt.has_annotations:
            return {}
        self.last = evaluate_ytvis(self.gt, self._mapped(), device=self.device, params=self.params,
                                   _counts=self._counts)
        return {"segm": self._derive(self.last)}
