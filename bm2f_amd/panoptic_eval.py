"""Panoptic quality (PQ) without panopticapi, detectron2 or PNG files: the role of detectron2's
``COCOPanopticEvaluator`` (attached by the reference's ``train_net.py:build_evaluator`` to every panoptic dataset) and
of panopticapi's ``pq_compute_single_core`` / ``PQStat.pq_average`` behind it.

panopticapi writes every prediction to a PNG, reads it back, and gets the pixels of every (ground-truth segment,
predicted segment) pair from ``np.unique`` on ``gt * 256^3 + pred``.  Here the head's id map stays on the device:
:func:`bm2f_amd.label_counts.label_pair_counts_ragged` counts a batch of images in one launch, in id-list mode (rows:
VOID, the image's ground-truth segment ids in ascending order, and "other"; columns: ``0 .. max predicted id``), and
only the tables reach the host.  :func:`pq_from_counts` then applies the matching rules to one table.

The rules, with ``area`` the row and column sums of the table and ``void[p] = table[VOID, p]``:

1. Preconditions, each a ``KeyError`` in panopticapi's wording: a non-zero predicted id that has pixels but no entry
   in ``segments_info``; an entry with no pixels; an entry whose category is unknown.
2. Every pair (g, p) with ``table[g, p] > 0``, g a listed non-crowd ground-truth segment, p a listed prediction and
   equal categories, visited in ascending (ground-truth id, predicted id) order: ``iou = table[g, p] / (area_p +
   area_g - table[g, p] - void[p])`` in fp64; if ``iou > 0.5`` the category's ``tp += 1``, ``iou += iou`` and both
   are matched.
3. Every unmatched non-crowd g adds ``fn`` to its category; a crowd g is remembered per category, the last one in
   ``segments_info`` order winning.
4. Every unmatched p adds ``fp`` to its category unless ``(void[p] + table[crowd of p's category, p]) / area_p > 0.5``.
5. Pixels of the "other" row (a ground-truth value that is neither VOID nor a listed segment) only enter ``area_p``.

The per-image statistics are added category by category in the order the images are processed, so the fp64 ``iou``
sums are reproducible.  Averaging is ``PQStat.pq_average`` over All, Things and Stuff.  panopticapi itself has not
been run against this module; its rules are checked against the reference's own ``pq_compute_single_image`` on
semantic maps (tests/golden/gen_seg_eval_golden.py) and against a dense per-pixel restatement (tests/pq_ref.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .label_counts import MAX_IDS, label_pair_counts_ragged
from .label_planes import as_label_plane, integer_plane, same_dtype

VOID = 0
MAX_PRED_ID = 65536                    # columns are 0 .. the largest predicted id: (1025 rows) x 2^16 counters at most


def rgb2id(color):
    """panopticapi's ``rgb2id``: ``R + 256 G + 256^2 B`` of an (H, W, 3) array (-> int32 (H, W)) or of one colour."""
    if isinstance(color, np.ndarray) and color.ndim == 3:
        c = color.astype(np.int32)
        return c[:, :, 0] + 256 * c[:, :, 1] + 256 * 256 * c[:, :, 2]
    return int(color[0] + 256 * color[1] + 256 * 256 * color[2])


def id2rgb(id_map):
    """panopticapi's ``id2rgb``: an integer (H, W) array -> (H, W, 3) uint8, one id -> ``[R, G, B]``."""
    if isinstance(id_map, np.ndarray):
        rest = id_map.copy()
        out = np.zeros(tuple(id_map.shape) + (3,), dtype=np.uint8)
        for i in range(3):
            out[..., i] = rest % 256
            rest //= 256
        return out
    color = []
    for _ in range(3):
        color.append(int(id_map) % 256)
        id_map = int(id_map) // 256
    return color


def _categories(categories):
    """-> {id: {"id", "isthing", ...}} from that dict or from the list of a COCO panoptic json."""
    if isinstance(categories, dict):
        return categories
    return {c["id"]: c for c in categories}


class PQStat:
    """Four counters per category (``tp``, ``fp``, ``fn`` int64 and the fp64 ``iou`` sum) and ``+=``, as
    panopticapi's class of that name; the categories are fixed at construction."""

    def __init__(self, category_ids):
        self.category_ids = list(category_ids)
        self.index = {c: i for i, c in enumerate(self.category_ids)}
        n = len(self.category_ids)
        self.tp, self.fp, self.fn = (np.zeros(n, dtype=np.int64) for _ in range(3))
        self.iou = np.zeros(n, dtype=np.float64)

    def __iadd__(self, other):
        if other.category_ids != self.category_ids:
            raise ValueError("statistics over different categories")
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        self.iou += other.iou
        return self

    def as_dict(self):
        return {c: {"tp": int(self.tp[i]), "fp": int(self.fp[i]), "fn": int(self.fn[i]), "iou": float(self.iou[i])}
                for c, i in self.index.items()}

    def pq_average(self, categories, isthing=None):
        """-> ({"pq", "sq", "rq", "n"}, {category: {"pq", "sq", "rq"}}) over the categories of the group (all, or
        those whose ``isthing`` equals the argument).  A category without tp, fp and fn is left out (its per-class
        entry is zeros); an empty group averages to NaN."""
        categories = _categories(categories)
        pq = sq = rq = 0.0
        n = 0
        per_class = {}
        for label, info in categories.items():
            if isthing is not None and (info["isthing"] == 1) != isthing:
                continue
            i = self.index[label]
            tp, fp, fn, iou = int(self.tp[i]), int(self.fp[i]), int(self.fn[i]), float(self.iou[i])
            if tp + fp + fn == 0:
                per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
                continue
            n += 1
            pq_class = iou / (tp + 0.5 * fp + 0.5 * fn)
            sq_class = iou / tp if tp != 0 else 0.0
            rq_class = tp / (tp + 0.5 * fp + 0.5 * fn)
            per_class[label] = {"pq": pq_class, "sq": sq_class, "rq": rq_class}
            pq += pq_class
            sq += sq_class
            rq += rq_class
        if n == 0:
            return {"pq": float("nan"), "sq": float("nan"), "rq": float("nan"), "n": 0}, per_class
        return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


def pq_from_counts(table, gt_segments, pred_segments, categories, *, gt_rows=None, void_row=0, void_col=VOID,
                   image_id=None) -> PQStat:
    """One image's table of pixel counts -> its :class:`PQStat` by the rules of the module's docstring.

    table (rows, cols): ``table[r, p]`` is the number of pixels of ground-truth row ``r`` and predicted id ``p``.
    gt_segments: dicts with ``id``, ``category_id`` and ``iscrowd`` (default 0); segment k lies in row ``gt_rows[k]``
    (default ``k + 1``, rows ascending with the id) and VOID in ``void_row`` (None: no VOID row); any other row is
    "other".  pred_segments: dicts with ``id`` (the column) and ``category_id``.  ``void_col`` is the predicted id
    that may have pixels without being listed (None: every predicted id must be listed).  categories: ``{id: {"id",
    "isthing"}}`` or the list of those dicts."""
    categories = _categories(categories)
    table = np.asarray(table, dtype=np.int64)
    rows, cols = table.shape
    stat = PQStat(sorted(categories))
    area_g, area_p = table.sum(1), table.sum(0)
    void = table[void_row] if void_row is not None else np.zeros(cols, dtype=np.int64)
    listed = {int(s["id"]): s for s in pred_segments}
    for p in np.flatnonzero(area_p).tolist():
        if p not in listed:
            if void_col is not None and p == void_col:
                continue
            raise KeyError("In the image with ID {} segment with ID {} is presented in PNG and not presented in "
                           "JSON.".format(image_id, p))
        if listed[p]["category_id"] not in categories:
            raise KeyError("In the image with ID {} segment with ID {} has unknown category_id {}.".format(
                image_id, p, listed[p]["category_id"]))
    absent = [p for p in listed if not 0 <= p < cols or area_p[p] == 0]
    if absent:
        raise KeyError("In the image with ID {} the following segment IDs {} are presented in JSON and not presented "
                       "in PNG.".format(image_id, absent))

    if gt_rows is None:
        gt_rows = range(1, len(gt_segments) + 1)
    seg_of_row = {int(r): s for r, s in zip(gt_rows, gt_segments)}
    row_of_seg = {id(s): int(r) for r, s in zip(gt_rows, gt_segments)}
    gt_matched, pred_matched = set(), set()
    for g, p in zip(*(x.tolist() for x in np.nonzero(table))):       # row-major: ascending (gt id, predicted id)
        seg, pred = seg_of_row.get(g), listed.get(p)
        if seg is None or pred is None or seg.get("iscrowd", 0) == 1 or seg["category_id"] != pred["category_id"]:
            continue
        inter = table[g, p]
        union = area_p[p] + area_g[g] - inter - void[p]
        iou = np.float64(inter) / np.float64(union)
        if iou > 0.5:
            c = stat.index[seg["category_id"]]
            stat.tp[c] += 1
            stat.iou[c] += iou
            gt_matched.add(g)
            pred_matched.add(p)

    crowd_row = {}
    for seg in gt_segments:
        g = row_of_seg[id(seg)]
        if g in gt_matched:
            continue
        if seg.get("iscrowd", 0) == 1:
            crowd_row[seg["category_id"]] = g                         # the last crowd of a category wins
            continue
        stat.fn[stat.index[seg["category_id"]]] += 1
    for p, pred in listed.items():
        if p in pred_matched:
            continue
        inter = void[p]
        if pred["category_id"] in crowd_row:
            inter = inter + table[crowd_row[pred["category_id"]], p]
        if np.float64(inter) / np.float64(area_p[p]) > 0.5:
            continue
        stat.fp[stat.index[pred["category_id"]]] += 1
    return stat


# -------------------------------------------------------------------------------------------------------------------
# ground truth
# -------------------------------------------------------------------------------------------------------------------
class PanopticGroundTruth:
    """A COCO panoptic json (``categories`` with ``id`` and ``isthing``; ``annotations`` with ``image_id``,
    ``file_name`` and ``segments_info`` of ``id``, ``category_id``, ``iscrowd``) and the id map of every image:
    ``id_maps[image_id]``, an integer (H, W) array or tensor of segment ids (a HIP tensor is used where it lies), or
    else the PNG ``png_root/file_name`` read with PIL and :func:`rgb2id` when the image is first needed."""

    def __init__(self, json_dict, id_maps=None, png_root=None):
        self.categories = {c["id"]: {**c, "isthing": int(c.get("isthing", 0))} for c in json_dict["categories"]}
        self.annotations = {}
        for ann in json_dict["annotations"]:
            segs = [{"id": int(s["id"]), "category_id": s["category_id"], "iscrowd": int(s.get("iscrowd", 0))}
                    for s in ann["segments_info"]]
            for s in segs:
                if not 0 < s["id"] < 2 ** 24:
                    raise ValueError(f"image {ann['image_id']}: segment id {s['id']} outside (0, 2^24)")
            if len({s["id"] for s in segs}) != len(segs):
                raise ValueError(f"image {ann['image_id']}: a segment id is listed twice")
            if len(segs) + 1 > MAX_IDS:
                raise ValueError(f"image {ann['image_id']}: {len(segs)} segments, at most {MAX_IDS - 1} fit the kernel's "
                                 "id list")
            self.annotations[ann["image_id"]] = {"file_name": ann.get("file_name"), "segments_info": segs}
        self.id_maps = dict(id_maps) if id_maps is not None else {}
        self.png_root = png_root

    def image_ids(self):
        return sorted(self.annotations)

    def segments(self, image_id):
        if image_id not in self.annotations:
            raise KeyError(f"the ground truth holds no image {image_id!r}")
        return self.annotations[image_id]["segments_info"]

    def id_map(self, image_id):
        """-> the image's id map as an int32 array or tensor."""
        if image_id in self.id_maps:
            m = self.id_maps[image_id]
        else:
            ann = self.annotations[image_id]
            if self.png_root is None or ann["file_name"] is None:
                raise KeyError(f"no id map for image {image_id!r}: pass id_maps or png_root")
            from PIL import Image                                     # only this route needs PIL
            with Image.open(os.path.join(self.png_root, ann["file_name"])) as im:
                m = rgb2id(np.asarray(im.convert("RGB"), dtype=np.uint8))
        m = integer_plane(m, f"image {image_id!r}: the id map")
        return m.to(torch.int32) if torch.is_tensor(m) else m.astype(np.int32)


# -------------------------------------------------------------------------------------------------------------------
# evaluation
# -------------------------------------------------------------------------------------------------------------------
def panoptic_counts(gt, items, device=None, path="auto"):
    """items: ``(image_id, id_map, segments_info)`` per image, ``segments_info`` with dataset category ids.  -> one
    ``(table, gt_segments, gt_rows)`` per image: one launch of the counting kernel for the whole batch (the numpy
    definition when no plane is on a HIP device).  Raises KeyError in panopticapi's wording when a predicted id map
    holds an id beyond those listed."""
    a_planes, b_planes, id_lists, rows, cols, metas = [], [], [], [], [], []
    for image_id, id_map, segments_info in items:
        segs = gt.segments(image_id)
        a = gt.id_map(image_id)
        b = as_label_plane(id_map, "panoptic_seg", wide=True)
        if device is not None:
            b = (b if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b))).to(device)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"image {image_id!r}: the prediction is {tuple(b.shape)}, the ground truth {tuple(a.shape)}")
        order = sorted(range(len(segs)), key=lambda k: segs[k]["id"])
        ids = [VOID] + [segs[k]["id"] for k in order]
        gt_rows = np.zeros(len(segs), dtype=np.int64)
        gt_rows[order] = np.arange(1, len(segs) + 1)
        top = max([int(s["id"]) for s in segments_info] + [0])
        if top >= MAX_PRED_ID:
            raise ValueError(f"image {image_id!r}: predicted segment id {top}: the table has one column per id up to "
                             f"the largest, so predicted ids must stay below {MAX_PRED_ID}; number the predicted "
                             "segments 1, 2, ... as the head does (ground-truth ids may be any value below 2^24)")
        a_planes.append(a)
        b_planes.append(b)
        id_lists.append(ids)
        rows.append(len(ids) + 1)
        cols.append(top + 1)
        metas.append((image_id, segs, gt_rows))
    if not metas:
        return []
    tables, bad = label_pair_counts_ragged(same_dtype(a_planes), same_dtype(b_planes), rows=rows, cols=cols,
                                           ids=id_lists, path=path)
    for k in np.flatnonzero(bad).tolist():
        # the error path alone reads a prediction back: name the first id that is not a column
        image_id = metas[k][0]
        b = b_planes[k]
        flat = (b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).reshape(-1).astype(np.int64)
        label = int(np.unique(flat[(flat < 0) | (flat >= cols[k])])[0])
        raise KeyError("In the image with ID {} segment with ID {} is presented in PNG and not presented in "
                       "JSON.".format(image_id, label))
    return [(t, segs, gt_rows) for t, (_, segs, gt_rows) in zip(tables, metas)]


class PanopticEvalResult(dict):
    """The metrics of :func:`evaluate_panoptic` (percent) with ``stat``, the accumulated :class:`PQStat`."""
    stat = None


def summarize_pq(stat, categories, class_names=None):
    """-> PQ, SQ, RQ (and ``_th``, ``_st``) x 100, ``n`` per group, ``per_class`` and the per-category ``stats``."""
    categories = _categories(categories)
    out = PanopticEvalResult()
    out.stat = stat
    for suffix, isthing in (("", None), ("_th", True), ("_st", False)):
        avg, per_class = stat.pq_average(categories, isthing=isthing)
        for k in ("pq", "sq", "rq"):
            out[k.upper() + suffix] = avg[k] * 100
        out["n" + suffix] = avg["n"]
        if isthing is None:
            out["per_class"] = {c: {k: v * 100 for k, v in r.items()} for c, r in per_class.items()}
    out["stats"] = stat.as_dict()
    return out


def evaluate_panoptic(gt, predictions, device=None, batch_size=16, path="auto") -> PanopticEvalResult:
    """gt: a :class:`PanopticGroundTruth`; predictions: ``(image_id, id_map, segments_info)`` per image with dataset
    category ids, counted ``batch_size`` images per launch on the device of the id maps (or ``device``).  Predicted
    segment ids must be small integers (below ``MAX_PRED_ID``; the head numbers them 1, 2, ...): an image's table
    has one column per id up to its largest.  Ground-truth ids may be any ``R + 256 G + 256^2 B`` value."""
    stat = PQStat(sorted(gt.categories))
    predictions = list(predictions)
    for k in range(0, len(predictions), batch_size):
        batch = predictions[k:k + batch_size]
        for (image_id, _, segments_info), (table, segs, gt_rows) in zip(batch, panoptic_counts(gt, batch, device, path)):
            stat += pq_from_counts(table, segs, segments_info, gt.categories, gt_rows=gt_rows, image_id=image_id)
    return summarize_pq(stat, gt.categories)


class COCOPanopticEvaluator:
    """detectron2's ``COCOPanopticEvaluator`` without detectron2, panopticapi or PNG files: ``reset()``,
    ``process(inputs, outputs)`` per batch and ``evaluate()``.

    ``process`` takes ``inputs[i]["image_id"]`` and ``outputs[i]["panoptic_seg"] = (id_map, segments_info)`` as
    :class:`MaskFormerInference` returns it.  A segment's contiguous ``category_id`` is mapped back to the dataset id
    through ``thing_dataset_id_to_contiguous_id`` or ``stuff_dataset_id_to_contiguous_id`` by its ``isthing``
    (detectron2's ``_convert_category_id``; a segment without ``isthing`` already carries a dataset id).  Every call
    is one launch of the counting kernel on the device of the id maps (or ``device``, to which host maps are then
    uploaded); the id maps are never copied to the host and nothing is written to disk."""

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id, stuff_dataset_id_to_contiguous_id,
                 device=None):
        self.gt = ground_truth if isinstance(ground_truth, PanopticGroundTruth) else PanopticGroundTruth(ground_truth)
        self._thing = {v: k for k, v in dict(thing_dataset_id_to_contiguous_id or {}).items()}
        self._stuff = {v: k for k, v in dict(stuff_dataset_id_to_contiguous_id or {}).items()}
        self.device = torch.device(device) if device is not None else None
        self.reset()

    def reset(self):
        self.stat = PQStat(sorted(self.gt.categories))
        self.num_images = 0

    def _convert(self, seg):
        seg = dict(seg)
        isthing = seg.pop("isthing", None)
        if isthing is None:
            return seg
        table = self._thing if isthing else self._stuff
        if seg["category_id"] not in table:
            raise KeyError(f"segment {seg.get('id')} has contiguous category {seg['category_id']}, which the "
                           f"{'thing' if isthing else 'stuff'} mapping does not hold")
        seg["category_id"] = table[seg["category_id"]]
        return seg

    def process(self, inputs, outputs):
        items = []
        for inp, out in zip(inputs, outputs):
            id_map, segments_info = out["panoptic_seg"]
            if segments_info is None:
                raise ValueError("panoptic_seg without segments_info is not supported")
            items.append((inp["image_id"], id_map, [self._convert(s) for s in segments_info]))
        for (image_id, _, segs_p), (table, segs_g, gt_rows) in zip(items, panoptic_counts(self.gt, items, self.device)):
            self.stat += pq_from_counts(table, segs_g, segs_p, self.gt.categories, gt_rows=gt_rows, image_id=image_id)
            self.num_images += 1

    def evaluate(self):
        """-> ``{"panoptic_seg": {"PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st", "n", "n_th",
        "n_st", "per_class", "stats"}}`` in percent; NaN for a group without a counted category."""
        return {"panoptic_seg": summarize_pq(self.stat, self.gt.categories)}
