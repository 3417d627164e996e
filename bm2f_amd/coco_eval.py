"""COCO instance AP for images: what the reference's ``InstanceSegEvaluator`` (mask2former/evaluation/
instance_evaluation.py:30-107) gets from ``pycocotools.cocoeval.COCOeval``, restated without pycocotools and
detectron2 on the list ``instances_to_coco_json`` writes.

``COCOeval`` and the reference's ``YTVOSeval`` (ytvis_api/ytvoseval.py) are one algorithm, the second being a copy of
the first with ``image`` renamed ``video``; the matching, accumulation and summary are those of ``bm2f_amd.ap_eval``,
shared with the video evaluator, and only what differs for images is written here:

  * the IoU of a detection with a crowd ground truth is ``i / area(detection)`` (``maskUtils.iou(d, g, iscrowd)``);
  * a ground truth's area is its annotation's ``area`` field, a detection's is its mask area (``segm``) or
    ``w * h`` (``bbox``), as ``COCO.loadRes`` sets them;
  * a ground truth is ignored exactly when ``iscrowd`` is set; detection ids are ``index + 1``;
  * the area ranges are all / small < 32^2 / medium / large >= 96^2.

The mask work is batched over images of different sizes: the images are cut into batches whose bit planes fit
``batch_bytes``, and a batch costs one upload, one launch of the ragged RLE decoder, one call of the ragged pair
counts and one device-to-host copy (``mask_iou.rle_pair_counts_ragged``), whatever the number of images in it.

Ground-truth segmentations are RLE (compressed, or uncompressed as COCO stores crowds).  Polygons raise
``NotImplementedError`` by default, because a different rasteriser would change AP silently: convert the file once
beforehand (``bm2f_amd.polygon.convert_polygons_to_rle``, or the rasteriser the numbers are to be compared with), or
pass ``polygons="rasterize"``.  Then a batch's RLE masks and polygon annotations go into one ragged buffer
(``polygon.pair_counts_ragged``): still one upload, one copy and a number of launches that does not depend on the
batch.  The rasteriser is ``bm2f_amd.polygon``'s restatement of ``rleFrPoly``; it has not been run against
pycocotools itself.  A batch without polygons takes the RLE path unchanged.

``iou_type="boundary"`` is Boundary AP: the IoU of a pair is the smaller of its mask IoU and the IoU of the two
masks' boundaries (``bm2f_amd.mask_boundary`` restates the definition and holds the batch step, which adds one launch
of the boundary kernel and a second pair count to the launches above).
"""
from __future__ import annotations

import copy
import json

import numpy as np

from .ap_eval import IMAGE, APEvaluator, EvalResult, evaluate_units, normalize_params
from .evaluation import instances_to_coco_json
from .mask_boundary import boundary_dilation, boundary_pair_counts_ragged, boundary_tiles
from .mask_iou import MAX_RAGGED_WORDS, rle_pair_counts_ragged
from .polygon import check_annotation, is_polygon, pair_counts_ragged

DEFAULT_BATCH_BYTES = 64 << 20
"""Bit planes per batch.  A COCO val image with 100 detections and 7 ground truths is ~107 planes of ~38 KB, about
4 MB, so 64 MiB holds some 16 images: enough for the per-batch host work (one upload, three launches, one copy) to
be shared by thousands of planes, small enough to stay inside the 256 MB last-level cache between the decoder's
stores and the pair kernel's loads."""


class COCOParams:
    """``Params.setDetParams`` of cocoeval.py."""

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


class COCOGroundTruth:
    """A COCO instances file (or the dict it holds): ``images``, ``annotations`` and ``categories`` indexed as
    ``pycocotools.coco.COCO`` does.  A segmentation is a compressed or an uncompressed RLE dict; a polygon raises
    NotImplementedError with ``polygons="refuse"`` (the default) and is kept, to be rasterised by the evaluation, with
    ``polygons="rasterize"`` (see the module docstring)."""

    def __init__(self, dataset, polygons="refuse"):
        if polygons not in ("refuse", "rasterize"):
            raise ValueError("polygons must be 'refuse' or 'rasterize'")
        self.polygons = polygons
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
            if seg is not None and not isinstance(seg, dict) and polygons == "refuse":
                raise NotImplementedError(
                    f"annotation {ann.get('id')} holds a polygon segmentation: convert the file to RLE once "
                    "beforehand (polygons are not rasterised here)")
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)

    def image_ids(self):
        return list(self.imgs.keys())

    def category_ids(self):
        return [c["id"] for c in self.dataset.get("categories", [])]


class COCOEvalResult(EvalResult):
    """What ``COCOeval`` holds after ``evaluate()``, ``accumulate()`` and ``summarize()``."""


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
            if what == "annotation" and gt.polygons == "rasterize" and is_polygon(seg):
                check_annotation(seg, f"annotation {r.get('id')}")
                continue
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


def _segm_counts(gt, img_ids, dets_of, device, batch_bytes, dilation_ratio=None):
    """-> {image id: (inter (D, G), area_d (D,), area_g (G,))} over all categories, G in the order of
    ``gt.img_to_anns``.  With a ``dilation_ratio`` (Boundary AP) -> that dict and the same of the masks' boundaries;
    a batch then holds a second buffer of boundary planes, so it takes half of ``batch_bytes`` of mask planes."""
    counts, edge_counts = {}, {}
    for img_id in img_ids:                                            # every check before the first launch
        _check_segm(gt, img_id, dets_of.get(img_id, []), gt.img_to_anns.get(img_id, []))
    if dilation_ratio is not None:
        d_max = boundary_tiles()[2]
        for img_id in img_ids:
            img = gt.imgs[img_id]
            if dets_of.get(img_id) or gt.img_to_anns.get(img_id):
                d = boundary_dilation(img["height"], img["width"], dilation_ratio)
                if d > d_max:
                    raise ValueError(f"image {img_id}: a dilation of {d} pixels is more than the {d_max} supported")
        batch_bytes = max(int(batch_bytes) // 2, 1)
    for batch in image_batches(gt, img_ids, dets_of, batch_bytes):
        rles, groups, sizes, names = [], [], [], []
        for img_id in batch:
            dets, anns = dets_of.get(img_id, []), gt.img_to_anns.get(img_id, [])
            n0 = len(rles)
            rles += [r["segmentation"] for r in dets] + [a["segmentation"] for a in anns]
            img = gt.imgs[img_id]
            size = (int(img["height"]), int(img["width"]))
            sizes += [None] * len(dets) + [size if is_polygon(a["segmentation"]) else None for a in anns]
            names += [None] * len(dets) + [f"annotation {a.get('id')}" for a in anns]
            groups.append((size[0], size[1], np.arange(n0, n0 + len(dets)),
                           np.arange(n0 + len(dets), n0 + len(dets) + len(anns))))
        if dilation_ratio is not None:
            batch_counts, batch_edges = boundary_pair_counts_ragged(rles, groups, device=device, sizes=sizes,
                                                                    names=names, dilation_ratio=dilation_ratio)
            edge_counts.update(zip(batch, batch_edges))
        elif any(s is not None for s in sizes):                       # polygon ground truth in this batch
            batch_counts = pair_counts_ragged(rles, groups, device=device, sizes=sizes, names=names)
        else:
            batch_counts = rle_pair_counts_ragged(rles, groups, device=device)
        for img_id, c in zip(batch, batch_counts):
            counts[img_id] = c
    return counts if dilation_ratio is None else (counts, edge_counts)


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
                  batch_bytes=DEFAULT_BATCH_BYTES, dilation_ratio=0.02) -> COCOEvalResult:
    """gt: a :class:`COCOGroundTruth`; results: the list ``instances_to_coco_json`` writes (``image_id``,
    ``category_id``, ``score``, ``segmentation`` as RLE, ``bbox`` as xywh).  ``iou_type`` is ``"segm"`` (masks, built
    and counted on ``device`` in batches of ``batch_bytes`` of planes), ``"boundary"`` or ``"bbox"`` (numpy).  Only
    ``useCats=1``.

    ``"boundary"`` is Boundary AP (``COCOeval`` of the boundary-iou-api with ``iouType="boundary"``, restated in
    ``bm2f_amd.mask_boundary``; that package has not been run against this code): the IoU of a pair is
    ``min(mask IoU, IoU of the two masks' boundaries)`` with ``d`` from ``dilation_ratio`` and each image's size, both
    with the crowd rule; everything else is as for ``"segm"`` (areas are mask areas, ``bbox`` fields are ignored).
    The boundary planes are a second buffer in every batch, counted in ``batch_bytes``.

    The rules (ordering, the ``maxDets[-1]`` cut per (image, category), matching thresholds and ties, the crowd
    re-match, the break on ignore, float32 accumulation, the -1 conventions, the 12 statistics) are listed in
    ``bm2f_amd.ap_eval``, with the COCO differences of the module docstring.

    Raises ValueError, before any launch, when a result names an unknown image, its mask size is not the image's, or
    (``bbox``) it has no ``bbox``."""
    if iou_type not in ("segm", "bbox", "boundary"):
        raise NotImplementedError("iou_type must be 'segm', 'boundary' or 'bbox'")
    p = normalize_params(IMAGE, params if params is not None else COCOParams(iou_type), gt.image_ids(),
                         gt.category_ids(), results, "results name images the ground truth does not hold")
    p.iouType = iou_type
    dets_of = {}
    for r in results:
        dets_of.setdefault(r["image_id"], []).append(r)
    second = None
    if iou_type == "segm":
        counts = _segm_counts(gt, p.imgIds, dets_of, device, batch_bytes)
    elif iou_type == "boundary":
        counts, edges = _segm_counts(gt, p.imgIds, dets_of, device, batch_bytes, dilation_ratio=float(dilation_ratio))
        second = lambda imgId, anns, dets: edges[imgId]               # noqa: E731
    else:
        counts = _bbox_counts(gt, p.imgIds, dets_of)
    return evaluate_units(p, IMAGE, gt.img_to_anns, results, lambda imgId, anns, dets: counts[imgId],
                          lambda ann: ann["area"], lambda r, area: area, crowd_iou=True, result_cls=COCOEvalResult,
                          second_counts_of=second)


# -------------------------------------------------------------------------------------------------------------------
# the evaluator
# -------------------------------------------------------------------------------------------------------------------
class COCOEvaluator(APEvaluator):
    """The reference's ``InstanceSegEvaluator`` without detectron2: ``reset()``, ``process(inputs, outputs)`` per
    batch of images and ``evaluate()``.

    ``process`` takes detectron2's pairs: ``inputs[i]["image_id"]`` and ``outputs[i]["instances"]``, the dict of
    :class:`MaskFormerInference` (``instance_rle=True`` or plain masks), written with ``instances_to_coco_json``.
    ``results`` is the accumulated ``coco_instances_results.json`` list with the head's contiguous category ids;
    ``evaluate`` maps them back through ``thing_dataset_id_to_contiguous_id`` (instance_evaluation.py:52-70).
    ``polygons`` is passed to :class:`COCOGroundTruth` when ``ground_truth`` is not one already.  ``tasks`` may hold
    ``"boundary"`` (Boundary AP with ``dilation_ratio``, see :func:`evaluate_coco`), reported under the same metric
    names."""

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id=None, class_names=None, device=None,
                 params=None, tasks=("segm",), batch_bytes=DEFAULT_BATCH_BYTES, polygons="refuse",
                 dilation_ratio=0.02):
        self.tasks = tuple(tasks)
        self.batch_bytes = batch_bytes
        self.dilation_ratio = dilation_ratio
        gt = (ground_truth if isinstance(ground_truth, COCOGroundTruth)
              else COCOGroundTruth(ground_truth, polygons=polygons))
        super().__init__(gt, thing_dataset_id_to_contiguous_id, class_names, device, params)

    def reset(self):
        super().reset()
        self.last = {}

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
            assert task in {"bbox", "segm", "boundary"}, f"Got unknown task: {task}!"
            if len(predictions) == 0:
                self.last[task] = None
            else:
                params = copy.deepcopy(self.params) if self.params is not None else None
                self.last[task] = evaluate_coco(self.gt, predictions, iou_type=task, device=self.device,
                                                params=params, batch_bytes=self.batch_bytes,
                                                dilation_ratio=self.dilation_ratio)
            out[task] = self._derive(self.last[task])
        return out
