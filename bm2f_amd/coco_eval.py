"""COCO instance AP for images: what the reference's ``InstanceSegEvaluator`` (mask2former/evaluation/
instance_evaluation.py:30-107) gets from ``pycocotools.cocoeval.COCOeval``, restated without pycocotools and
detectron2 on the list ``instances_to_coco_json`` writes.

``COCOeval`` and the reference's ``YTVOSeval`` (ytvis_api/ytvoseval.py) are one algorithm, the second being a copy of
the first with ``image`` renamed ``video``; so the matching, accumulation and summary are the functions of
``bm2f_amd.ytvis_eval``, imported and unchanged, and only what differs for images is written here:

  * the IoU of a detection with a crowd ground truth is ``i / area(detection)`` (``maskUtils.iou(d, g, iscrowd)``);
  * a ground truth's area is its annotation's ``area`` field, a detection's is its mask area (``segm``) or
    ``w * h`` (``bbox``), as ``COCO.loadRes`` sets them;
  * a ground truth is ignored exactly when ``iscrowd`` is set; detection ids are ``index + 1``;
  * the area ranges are all / small < 32^2 / medium / large >= 96^2.

The mask work is batched over images of different sizes: the images are cut into batches whose bit planes fit
``batch_bytes``, and a batch costs one upload, one launch of the ragged RLE decoder, one call of the ragged pair
counts and one device-to-host copy (``mask_iou.rle_pair_counts_ragged``), whatever the number of images in it.

Ground-truth segmentations must be RLE (compressed, or uncompressed as COCO stores crowds).  Polygons raise
``NotImplementedError``: they have to be converted to RLE once beforehand with the rasteriser the numbers are to be
compared with; a different rasteriser here would change AP silently.
"""
from __future__ import annotations

import copy
import json

import numpy as np

from .evaluation import instances_to_coco_json
from .mask_iou import MAX_RAGGED_WORDS, mask_iou, rle_pair_counts_ragged
from .ytvis_eval import _accumulate, _evaluate_vid, _sorted_dets, _summarize

DEFAULT_BATCH_BYTES = 64 << 20
"""Bit planes per batch.  A COCO val image with 100 detections and 7 ground truths is ~107 planes of ~38 KB, about
4 MB, so 64 MiB holds some 16 images: enough for the per-batch host work (one upload, three launches, one copy) to
be shared by thousands of planes, small enough to stay inside the 256 MB last-level cache between the decoder's
stores and the pair kernel's loads."""


class COCOParams:
    """``Params.setDetParams`` of cocoeval.py.  ``vidIds`` is ``imgIds`` under the name the shared functions read."""

    def __init__(self, iouType="segm"):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = iouType

    @property
    def vidIds(self):
        return self.imgIds


class COCOGroundTruth:
    """A COCO instances file (or the dict it holds): ``images``, ``annotations`` and ``categories`` indexed as
    ``pycocotools.coco.COCO`` does.  A segmentation is a compressed or an uncompressed RLE dict; a polygon raises
    NotImplementedError (see the module docstring)."""

    def __init__(self, dataset):
        if isinstance(dataset, (str, bytes)) or hasattr(dataset, "__fspath__"):
            with open(dataset) as f:
                dataset = json.load(f)
        if not isinstance(dataset, dict):
            raise ValueError("the ground truth must be a dict or the path of a JSON file holding one")
        self.dataset = dataset
        self.imgs = {im["id"]: im for im in dataset.get("images", [])}
        self.cats = {c["id"]: c for c in dataset.get("categories", [])}
        self.anns = list(dataset.get("annotations", []))
        self.has_annotations = "annotations" in dataset
        self.img_to_anns = {}
        for ann in self.anns:
            seg = ann.get("segmentation")
            if seg is not None and not isinstance(seg, dict):
                raise NotImplementedError(
                    f"annotation {ann.get('id')} holds a polygon segmentation: convert the file to RLE once "
                    "beforehand (polygons are not rasterised here)")
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)

    def image_ids(self):
        return list(self.imgs.keys())

    def category_ids(self):
        return [c["id"] for c in self.dataset.get("categories", [])]


class COCOEvalResult:
    """What ``COCOeval`` holds after ``evaluate()``, ``accumulate()`` and ``summarize()``: ``ious`` {(image,
    category): (D, G) array or []}, ``evalImgs`` (one record or None per category, area range and image, in that
    order), ``precision`` (T, R, K, A, M), ``recall`` (T, K, A, M), ``scores`` and the 12 ``stats``."""

    def __init__(self, params, ious, evalImgs, precision, recall, scores, stats):
        self.params, self.ious, self.evalImgs = params, ious, evalImgs
        self.precision, self.recall, self.scores, self.stats = precision, recall, scores, stats
        self.eval = {"params": params, "counts": list(precision.shape), "precision": precision, "recall": recall,
                     "scores": scores}


# -------------------------------------------------------------------------------------------------------------------
# counts: masks in batches on the device, boxes in numpy
# -------------------------------------------------------------------------------------------------------------------
def _plane_bytes(img):
    return 4 * int(img["height"]) * ((int(img["width"]) + 31) // 32)


def _check_segm(gt, img_id, dets, anns):
    img = gt.imgs[img_id]
    size = [int(img["height"]), int(img["width"])]
    for what, items in (("result", dets), ("annotation", anns)):
        for r in items:
            seg = r.get("segmentation")
            if not isinstance(seg, dict) or "size" not in seg or "counts" not in seg:
                raise ValueError(f"a {what} of image {img_id} has no RLE segmentation")
            if [int(v) for v in seg["size"]] != size:
                raise ValueError(f"a {what} of image {img_id} has size {list(seg['size'])}, the image is {size}")


def image_batches(gt, img_ids, dets_of, batch_bytes):
    """The images that have any mask, in order, cut so that the planes of a batch (padded to 16 bytes) fit
    ``batch_bytes``; an image larger than that is a batch of its own.  A batch never exceeds the 2^31 - 1 words of
    one ragged buffer, whatever ``batch_bytes`` says."""
    batch_bytes = min(int(batch_bytes), 4 * MAX_RAGGED_WORDS)
    batches, cur, used = [], [], 0
    for img_id in img_ids:
        n = len(dets_of.get(img_id, [])) + len(gt.img_to_anns.get(img_id, []))
        if n == 0:
            continue
        need = n * ((_plane_bytes(gt.imgs[img_id]) + 15) // 16 * 16)
        if cur and used + need > batch_bytes:
            batches.append(cur)
            cur, used = [], 0
        cur.append(img_id)
        used += need
    if cur:
        batches.append(cur)
    return batches


def _segm_counts(gt, img_ids, dets_of, device, batch_bytes):
    """-> {image id: (inter (D, G), area_d (D,), area_g (G,))} over all categories, G in the order of
    ``gt.img_to_anns``."""
    counts = {}
    for img_id in img_ids:                                            # every check before the first launch
        _check_segm(gt, img_id, dets_of.get(img_id, []), gt.img_to_anns.get(img_id, []))
    for batch in image_batches(gt, img_ids, dets_of, batch_bytes):
        rles, groups = [], []
        for img_id in batch:
            dets, anns = dets_of.get(img_id, []), gt.img_to_anns.get(img_id, [])
            n0 = len(rles)
            rles += [r["segmentation"] for r in dets] + [a["segmentation"] for a in anns]
            img = gt.imgs[img_id]
            groups.append((int(img["height"]), int(img["width"]), np.arange(n0, n0 + len(dets)),
                           np.arange(n0 + len(dets), n0 + len(dets) + len(anns))))
        for img_id, c in zip(batch, rle_pair_counts_ragged(rles, groups, device=device)):
            counts[img_id] = c
    return counts


def _xywh(items, what, img_id):
    for r in items:
        if "bbox" not in r or len(r["bbox"]) != 4:
            raise ValueError(f"a {what} of image {img_id} has no 'bbox'")
    return np.asarray([r["bbox"] for r in items], dtype=np.float64).reshape(-1, 4)


def _bbox_counts(gt, img_ids, dets_of):
    """The same triple from xywh boxes in float64 (``bbIou`` of maskApi.c: w * h areas, clipped overlaps)."""
    counts = {}
    for img_id in img_ids:
        dets, anns = dets_of.get(img_id, []), gt.img_to_anns.get(img_id, [])
        if not dets and not anns:
            continue
        d, g = _xywh(dets, "result", img_id), _xywh(anns, "annotation", img_id)
        w = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - \
            np.maximum(d[:, None, 0], g[None, :, 0])
        h = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - \
            np.maximum(d[:, None, 1], g[None, :, 1])
        counts[img_id] = (np.maximum(w, 0) * np.maximum(h, 0), d[:, 2] * d[:, 3], g[:, 2] * g[:, 3])
    return counts


# -------------------------------------------------------------------------------------------------------------------
# evaluate
# -------------------------------------------------------------------------------------------------------------------
def evaluate_coco(gt, results, iou_type="segm", device=None, params=None,
                  batch_bytes=DEFAULT_BATCH_BYTES) -> COCOEvalResult:
    """gt: a :class:`COCOGroundTruth`; results: the list ``instances_to_coco_json`` writes (``image_id``,
    ``category_id``, ``score``, ``segmentation`` as RLE, ``bbox`` as xywh).  ``iou_type`` is ``"segm"`` (masks, built
    and counted on ``device`` in batches of ``batch_bytes`` of planes) or ``"bbox"`` (numpy).  Only ``useCats=1``.

    The rules are those of ``evaluate_ytvis`` (ordering, the ``maxDets[-1]`` cut per (image, category), matching
    thresholds and ties, the crowd re-match, the break on ignore, float32 accumulation, the -1 conventions, the 12
    statistics) with the COCO differences listed in the module docstring.  An empty pair of one side keeps the
    ``(D, 0)`` / ``(0, G)`` IoU array of the shared code where ``maskUtils.iou`` returns ``[]``; no number depends
    on it.

    Raises ValueError, before any launch, when a result names an unknown image, its mask size is not the image's, or
    (``bbox``) it has no ``bbox``."""
    if iou_type not in ("segm", "bbox"):
        raise NotImplementedError("iou_type must be 'segm' or 'bbox'")
    p = copy.deepcopy(params) if params is not None else COCOParams(iou_type)
    p.iouType = iou_type
    if not p.useCats:
        raise NotImplementedError("only useCats=1 is supported")
    img_ids = p.imgIds if len(p.imgIds) else sorted(gt.image_ids())
    cat_ids = p.catIds if len(p.catIds) else sorted(gt.category_ids())
    p.imgIds = list(np.unique(img_ids))
    p.catIds = list(np.unique(cat_ids))
    p.maxDets = sorted(p.maxDets)
    maxDet = p.maxDets[-1]
    known = set(gt.image_ids())
    if any(r["image_id"] not in known for r in results):
        raise ValueError("results name images the ground truth does not hold")
    cats = set(p.catIds)

    dets_of = {}
    for index, r in enumerate(results):
        dets_of.setdefault(r["image_id"], []).append((index, r))
    plain = {k: [r for _, r in v] for k, v in dets_of.items()}
    if iou_type == "segm":
        counts = _segm_counts(gt, p.imgIds, plain, device, batch_bytes)
    else:
        counts = _bbox_counts(gt, p.imgIds, plain)

    gts_by, dts_by, ious = {}, {}, {}
    for imgId in p.imgIds:
        anns, dets = gt.img_to_anns.get(imgId, []), dets_of.get(imgId, [])
        inter, area_d, area_g = counts.get(imgId, (None, None, None))
        for j, ann in enumerate(anns):
            if ann["category_id"] in cats:
                gts_by.setdefault((imgId, ann["category_id"]), []).append(
                    {"id": ann["id"], "row": j, "iscrowd": ann.get("iscrowd", 0),
                     "ignore": bool(ann.get("iscrowd", 0)), "avg_area": ann["area"]})
        for i, (index, r) in enumerate(dets):
            if r["category_id"] in cats:
                dts_by.setdefault((imgId, r["category_id"]), []).append(
                    {"id": index + 1, "row": i, "score": r["score"], "avg_area": area_d[i]})
        for catId in p.catIds:
            g, d = gts_by.get((imgId, catId), []), dts_by.get((imgId, catId), [])
            if len(g) == 0 and len(d) == 0:
                ious[imgId, catId] = []
                continue
            d = _sorted_dets(d, maxDet)
            rows_d, rows_g = [x["row"] for x in d], [x["row"] for x in g]
            if not rows_d or not rows_g:
                ious[imgId, catId] = np.zeros([len(d), len(g)])
                continue
            ious[imgId, catId] = mask_iou(inter[np.ix_(rows_d, rows_g)], area_d[rows_d], area_g[rows_g],
                                          iscrowd=[x["iscrowd"] for x in g])

    evalImgs = [_evaluate_vid(p, gts_by.get((imgId, catId), []), dts_by.get((imgId, catId), []), ious[imgId, catId],
                              imgId, catId, aRng, maxDet)
                for catId in p.catIds for aRng in p.areaRng for imgId in p.imgIds]
    for e in evalImgs:
        if e is not None:
            e["image_id"] = e.pop("video_id")
    precision, recall, scores = _accumulate(p, evalImgs)
    return COCOEvalResult(p, ious, evalImgs, precision, recall, scores, _summarize(p, precision, recall))


# -------------------------------------------------------------------------------------------------------------------
# the evaluator
# -------------------------------------------------------------------------------------------------------------------
class COCOEvaluator:
    """The reference's ``InstanceSegEvaluator`` without detectron2: ``reset()``, ``process(inputs, outputs)`` per
    batch of images and ``evaluate()``.

    ``process`` takes detectron2's pairs: ``inputs[i]["image_id"]`` and ``outputs[i]["instances"]``, the dict of
    :class:`MaskFormerInference` (``instance_rle=True`` or plain masks), written with ``instances_to_coco_json``.
    ``results`` is the accumulated ``coco_instances_results.json`` list with the head's contiguous category ids;
    ``evaluate`` maps them back through ``thing_dataset_id_to_contiguous_id`` (instance_evaluation.py:52-70)."""

    METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10"]

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id=None, class_names=None, device=None,
                 params=None, tasks=("segm",), batch_bytes=DEFAULT_BATCH_BYTES):
        self.gt = ground_truth if isinstance(ground_truth, COCOGroundTruth) else COCOGroundTruth(ground_truth)
        self.id_map = thing_dataset_id_to_contiguous_id
        self.class_names = class_names
        self.device = device
        self.params = params
        self.tasks = tuple(tasks)
        self.batch_bytes = batch_bytes
        self.reset()

    def reset(self):
        self._predictions = []
        self.last = {}

    @property
    def results(self):
        return self._predictions

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            if "instances" in out:
                self._predictions.extend(instances_to_coco_json(out["instances"], inp["image_id"]))

    def _mapped(self):
        predictions = [dict(r) for r in self._predictions]
        if self.id_map is not None:
            reverse = {v: k for k, v in self.id_map.items()}
            for r in predictions:
                assert r["category_id"] in reverse, (
                    f"A prediction has class={r['category_id']}, but the dataset only has class ids in {self.id_map}.")
                r["category_id"] = reverse[r["category_id"]]
        return predictions

    def evaluate(self):
        """-> ``{task: {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AP-<name>", ...}}`` in percent, NaN where the
        summary is negative (detectron2's ``_derive_coco_results``); ``{}`` without annotations.  With an empty
        result list nothing is evaluated (the reference passes ``coco_eval=None``: "cocoapi does not handle empty
        results very well", instance_evaluation.py:100-101): ``last[task]`` is None and every metric NaN."""
        if not self.gt.has_annotations:
            return {}
        predictions = self._mapped()
        out = {}
        for task in sorted(self.tasks):
            assert task in {"bbox", "segm"}, f"Got unknown task: {task}!"
            if len(predictions) == 0:
                self.last[task] = None
                out[task] = {m: float("nan") for m in self.METRICS}
                continue
            params = copy.deepcopy(self.params) if self.params is not None else None
            r = evaluate_coco(self.gt, predictions, iou_type=task, device=self.device, params=params,
                              batch_bytes=self.batch_bytes)
            self.last[task] = r
            res = {m: float(r.stats[i] * 100 if r.stats[i] >= 0 else "nan") for i, m in enumerate(self.METRICS)}
            names = self.class_names
            if names is not None and len(names) > 1:
                assert len(names) == r.precision.shape[2]
                for idx, name in enumerate(names):
                    pr = r.precision[:, :, idx, 0, -1]
                    pr = pr[pr > -1]
                    res["AP-" + "{}".format(name)] = float(np.mean(pr) * 100) if pr.size else float("nan")
            out[task] = res
        return out
