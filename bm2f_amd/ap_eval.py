"""Instance AP on per-unit pair counts: the part ``pycocotools.cocoeval.COCOeval`` and the reference's ``YTVOSeval``
(mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py) share, the second being a copy of the first with
``image`` renamed ``video``.  A *unit* is what detections and ground truths are matched within: an image
(``coco_eval``) or a video (``ytvis_eval``).  No device code and no dataset knowledge here: an evaluator hands over,
per unit, its ground truths, its detections and the counts ``(inter (D, G), area_d, area_g)``, and says how the areas
of the records are filled.  ``file:line`` below are lines of ytvoseval.py unless a file is named.

Reference behaviours reproduced:
  * detection ids are ``index + 1`` in the results list (ytvos.py:249) and ``iscrowd = 0`` (ytvos.py:255);
  * a detection's ``avg_area`` is the mean of its per-frame mask areas without the zero-area and missing frames,
    ``l = [a for a in ann['areas'] if a]`` (ytvos.py:250-254); a ground truth's comes from its ``areas`` field
    the same way (:100-104); for images both are the single area ``COCO.loadRes`` and the annotation give;
  * a ground truth is ignored when it is a crowd (:120) or its ``avg_area`` is outside the area range (:283);
  * detections are ordered by score and ground truths by ignore flag with the stable mergesort (:186, :289, :291);
  * detections beyond ``maxDets[-1]`` per (unit, category) are dropped (:188-189, :292);
  * a match needs ``iou >= min(t, 1 - 1e-10)`` (:308) and a later ground truth wins ties (:318-322);
  * a matched ground truth is skipped unless it is a crowd, which may be matched again (:312);
  * the search stops at the first ignored ground truth once a regular one is matched (the break, :315);
  * a matched detection takes its ground truth's ignore flag (:326); an unmatched one is ignored when its
    ``avg_area`` is outside the area range (:330-331);
  * ``accumulate`` sums true and false positives in float32 (:410-411), divides by ``fp + tp + np.spacing(1)``
    (:417), makes precision monotone from the right (:430-432) and samples it with
    ``searchsorted(side="left")`` (:434), leaving 0 beyond the last recall;
  * precision, recall and scores are -1 for settings without ground truth (:366-368, :405), and a summary over
    no value is -1 (:484-485); ``stats[0]`` asks for ``maxDets == 100`` whatever ``params.maxDets`` holds (:492).
An empty pair of one side keeps a ``(D, 0)`` / ``(0, G)`` IoU array where ``maskUtils.iou`` returns ``[]``; no number
depends on it.
"""
from __future__ import annotations

import collections
import copy

import numpy as np

from .mask_iou import mask_iou

Unit = collections.namedtuple("Unit", "id_key ids_attr")
"""What names the unit: the key of a record (results, ``evalImgs``) and the params attribute holding the ids."""
IMAGE = Unit("image_id", "imgIds")
VIDEO = Unit("video_id", "vidIds")


class EvalResult:
    """What the reference evaluators hold after ``evaluate()``, ``accumulate()`` and ``summarize()``: ``ious`` {(unit,
    category): (D, G) array or []}, ``evalImgs`` (one record or None per category, area range and unit, in that
    order), ``precision`` (T, R, K, A, M), ``recall`` (T, K, A, M), ``scores`` and the 12 ``stats``."""

    def __init__(self, params, ious, evalImgs, precision, recall, scores, stats):
        self.params, self.ious, self.evalImgs = params, ious, evalImgs
        self.precision, self.recall, self.scores, self.stats = precision, recall, scores, stats
        self.eval = {"params": params, "counts": list(precision.shape), "precision": precision, "recall": recall,
                     "scores": scores}


def normalize_params(unit, params, gt_unit_ids, gt_cat_ids, results, unknown):
    """A private copy of ``params`` as the evaluation runs with it: unit and category ids default to the ground
    truth's and are made unique and sorted, ``maxDets`` is sorted.  Refuses ``useCats=0``, and results that name a unit
    the ground truth does not hold (ValueError with the evaluator's text ``unknown``)."""
    p = copy.deepcopy(params)
    if not p.useCats:
        raise NotImplementedError("only useCats=1 is supported")
    unit_ids = getattr(p, unit.ids_attr)
    setattr(p, unit.ids_attr, list(np.unique(unit_ids if len(unit_ids) else sorted(gt_unit_ids))))
    p.catIds = list(np.unique(p.catIds if len(p.catIds) else sorted(gt_cat_ids)))
    p.maxDets = sorted(p.maxDets)
    known = set(gt_unit_ids)
    if any(r[unit.id_key] not in known for r in results):
        raise ValueError(unknown)
    return p


def _sorted_dets(dt, max_det):
    inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
    return [dt[i] for i in inds[0:max_det]]


def _evaluate_unit(p, unit, gt, dt, ious_all, unitId, catId, aRng, maxDet):
    """``evaluateVid`` (:267-345) for the ground truths ``gt`` and detections ``dt`` of one (unit, category)."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    ignore = [1 if (g['ignore'] or (g['avg_area'] < aRng[0] or g['avg_area'] > aRng[1])) else 0 for g in gt]
    gtind = np.argsort(ignore, kind='mergesort')                      # ignored ground truths last, stable (:289)
    gt = [gt[i] for i in gtind]
    dt = _sorted_dets(dt, maxDet)                                     # highest score first, stable (:291-292)
    iscrowd = np.array([int(g['iscrowd']) for g in gt], dtype=bool)
    ious = ious_all[:, gtind] if len(ious_all) > 0 else ious_all
    T, G, D = len(p.iouThrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gtIg = np.array([ignore[i] for i in gtind])
    dtIg = np.zeros((T, D))
    if not len(ious) == 0:
        floor = np.minimum(np.asarray(p.iouThrs, dtype=np.float64), 1 - 1e-10)   # min([t, 1 - 1e-10]) (:308)
        gt_ids = np.array([g['id'] for g in gt])
        rows = np.arange(T)
        for dind, d in enumerate(dt):
            best = floor.copy()
            m = np.full(T, -1)
            stopped = np.zeros(T, dtype=bool)
            for gind in range(G):
                # matched already and not a crowd: skip (:312); a crowd can be matched again
                skip = (gtm[:, gind] > 0) & (not iscrowd[gind])
                # matched to a regular ground truth and now at an ignored one: stop (:315)
                if gtIg[gind] == 1:
                    stopped |= ~skip & (m > -1) & (gtIg[np.maximum(m, 0)] == 0)
                take = ~skip & ~stopped & ~(ious[dind, gind] < best)
                best[take] = ious[dind, gind]
                m[take] = gind
            hit = m > -1
            mh = m[hit]
            dtIg[hit, dind] = gtIg[mh]
            dtm[hit, dind] = gt_ids[mh]
            gtm[rows[hit], mh] = d['id']
    # unmatched detections outside the area range are ignored (:330-331)
    a = np.array([d['avg_area'] < aRng[0] or d['avg_area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {unit.id_key: unitId, 'category_id': catId, 'aRng': aRng, 'maxDet': maxDet,
            'dtIds': [d['id'] for d in dt], 'gtIds': [g['id'] for g in gt], 'dtMatches': dtm, 'gtMatches': gtm,
            'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}


def _accumulate(p, evalImgs, num_units):
    """``accumulate`` (:347-450) with the parameters the evaluation ran with."""
    T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
    precision = -np.ones((T, R, K, A, M))                             # -1 for absent settings (:366-368)
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    I0 = num_units
    for k in range(K):
        for a in range(A):
            for m, maxDet in enumerate(p.maxDets):
                E = [e for e in evalImgs[(k * A + a) * I0:(k * A + a + 1) * I0] if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')        # stable, as the reference (:398)
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float32)   # float32 sums (:410-411)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float32)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))               # (:417)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]    # the running maximum from the right (:430-432)
                    inds_r = np.searchsorted(rc, p.recThrs, side='left')
                    ok = inds_r < nd                                  # the reference's loop stops at the first miss
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    q[ok] = pr[inds_r[ok]]
                    ss[ok] = dtScoresSorted[inds_r[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return precision, recall, scores


def _summarize(p, precision, recall):
    """``summarize`` (:454-504): the 12 numbers; -1 where a setting has no value."""
    def one(ap=1, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        s = precision if ap == 1 else recall
        if iouThr is not None:
            s = s[np.where(iouThr == p.iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iouThr=.5, maxDets=p.maxDets[2])
    stats[2] = one(1, iouThr=.75, maxDets=p.maxDets[2])
    stats[3] = one(1, areaRng='small', maxDets=p.maxDets[2])
    stats[4] = one(1, areaRng='medium', maxDets=p.maxDets[2])
    stats[5] = one(1, areaRng='large', maxDets=p.maxDets[2])
    stats[6] = one(0, maxDets=p.maxDets[0])
    stats[7] = one(0, maxDets=p.maxDets[1])
    stats[8] = one(0, maxDets=p.maxDets[2])
    stats[9] = one(0, areaRng='small', maxDets=p.maxDets[2])
    stats[10] = one(0, areaRng='medium', maxDets=p.maxDets[2])
    stats[11] = one(0, areaRng='large', maxDets=p.maxDets[2])
    return stats


def evaluate_units(p, unit, anns_of, results, counts_of, gt_area, dt_area, crowd_iou, result_cls=EvalResult,
                   second_counts_of=None):
    """The evaluation proper with normalised params ``p``.  ``anns_of`` maps a unit id to its annotations;
    ``counts_of(unit id, annotations, results of the unit)`` gives ``(inter, area_d, area_g)`` over all categories, rows in
    the order of those two lists, and is asked only for units that hold anything; ``gt_area(annotation)`` and
    ``dt_area(result, its row of area_d)`` fill ``avg_area``.  With ``crowd_iou`` the IoU with a crowd ground truth is
    ``i / area(detection)`` (``maskUtils.iou(d, g, iscrowd)``).  ``second_counts_of``, where given, is asked like
    ``counts_of`` for a second triple (Boundary AP: the counts of the boundaries) and the IoU of a pair is the smaller
    of the two triples' IoUs, each with the crowd rule on its own areas; the areas handed to ``dt_area`` stay those
    of ``counts_of``.  -> ``result_cls`` (an :class:`EvalResult`)."""
    unit_ids, cats, maxDet = getattr(p, unit.ids_attr), set(p.catIds), p.maxDets[-1]
    dets_of = {}
    for index, r in enumerate(results):
        dets_of.setdefault(r[unit.id_key], []).append((index, r))
    gts_by, dts_by, ious = {}, {}, {}
    for unitId in unit_ids:
        anns, dets = anns_of.get(unitId, []), dets_of.get(unitId, [])
        if anns or dets:
            inter, area_d, area_g = counts_of(unitId, anns, [r for _, r in dets])
            if second_counts_of is not None:
                inter2, area_d2, area_g2 = second_counts_of(unitId, anns, [r for _, r in dets])
        for j, ann in enumerate(anns):
            if ann["category_id"] in cats:
                gts_by.setdefault((unitId, ann["category_id"]), []).append(
                    {"id": ann["id"], "row": j, "iscrowd": ann.get("iscrowd", 0),
                     "ignore": bool(ann.get("iscrowd", 0)), "avg_area": gt_area(ann)})
        for i, (index, r) in enumerate(dets):
            if r["category_id"] in cats:
                dts_by.setdefault((unitId, r["category_id"]), []).append(
                    {"id": index + 1, "row": i, "score": r["score"], "avg_area": dt_area(r, area_d[i])})
        for catId in p.catIds:
            g, d = gts_by.get((unitId, catId), []), dts_by.get((unitId, catId), [])
            if len(g) == 0 and len(d) == 0:
                ious[unitId, catId] = []
                continue
            d = _sorted_dets(d, maxDet)
            rows_d, rows_g = [x["row"] for x in d], [x["row"] for x in g]
            if not rows_d or not rows_g:
                ious[unitId, catId] = np.zeros([len(d), len(g)])
                continue
            crowd = [x["iscrowd"] for x in g] if crowd_iou else None
            ious[unitId, catId] = mask_iou(inter[np.ix_(rows_d, rows_g)], area_d[rows_d], area_g[rows_g], iscrowd=crowd)
            if second_counts_of is not None:
                ious[unitId, catId] = np.minimum(ious[unitId, catId], mask_iou(
                    inter2[np.ix_(rows_d, rows_g)], area_d2[rows_d], area_g2[rows_g], iscrowd=crowd))

    evalImgs = [_evaluate_unit(p, unit, gts_by.get((unitId, catId), []), dts_by.get((unitId, catId), []),
                               ious[unitId, catId], unitId, catId, aRng, maxDet)
                for catId in p.catIds for aRng in p.areaRng for unitId in unit_ids]
    precision, recall, scores = _accumulate(p, evalImgs, len(unit_ids))
    return result_cls(p, ious, evalImgs, precision, recall, scores, _summarize(p, precision, recall))


class APEvaluator:
    """What the image and the video evaluator share: the accumulated ``results`` list with the head's contiguous
    category ids and the metrics of an :class:`EvalResult` as detectron2's ``_derive_coco_results`` reports them."""

    METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10"]

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id, class_names, device, params):
        self.gt = ground_truth
        self.id_map = thing_dataset_id_to_contiguous_id
        self.class_names = class_names
        self.device = device
        self.params = params
        self.reset()

    def reset(self):
        self._predictions = []

    @property
    def results(self):
        return self._predictions

    def _derive(self, result):
        """-> {"AP", "AP50", ..., "AR10", "AP-<name>", ...} in percent, NaN where the summary is negative; every
        metric NaN for ``result=None`` (nothing was evaluated)."""
        if result is None:
            return {m: float("nan") for m in self.METRICS}
        stats = result.stats
        res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(self.METRICS)}
        names = self.class_names
        if names is not None and len(names) > 1:
            assert len(names) == result.precision.shape[2]
            for idx, name in enumerate(names):
                pr = result.precision[:, :, idx, 0, -1]
                pr = pr[pr > -1]
                res["AP-" + "{}".format(name)] = float(np.mean(pr) * 100) if pr.size else float("nan")
        return res
