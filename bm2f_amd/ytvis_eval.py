"""Video instance AP: the reference's ``YTVISEvaluator.evaluate()`` (mask2former_video/data_video/ytvis_eval.py:115-253)
and what it drives, ``YTVOS`` (data_video/datasets/ytvis_api/ytvos.py) and ``YTVOSeval`` (ytvis_api/ytvoseval.py),
restated without pycocotools and detectron2.  ``file:line`` below are lines of ytvoseval.py unless a file is named.

The mask work (the reference's ``computeIoU``, :176-222: one ``pycocotools.mask.merge`` and ``area`` per detection,
ground truth and frame) runs on bit planes: per video, every ground-truth frame and every detection frame becomes a
plane (``rle_to_bits``, or the head's ``pred_bits``), one ``mask_pair_counts`` launch counts all pairs of the video
over all categories, and the host slices by category.  A missing frame (``None``) is a zero plane on either side, which
is what the three branches of ``iou_seq`` (:203-217) add up to: ``i = sum |d & g|``, ``u = sum |d| + sum |g| - i``.

Matching, accumulation and the summary stay on the host in numpy, vectorised over the IoU thresholds; they handle at
most ``maxDets[-1]`` detections times a handful of objects per (video, category) and are not the hot path.
"""
from __future__ import annotations

import copy
import json

import numpy as np
import torch

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


class YTVISEvalResult:
    """What ``YTVOSeval`` holds after ``evaluate()``, ``accumulate()`` and ``summarize()``: ``ious`` {(video, category):
    (D, G) array or []}, ``evalImgs`` (one record or None per category, area range and video, in that order),
    ``precision`` (T, R, K, A, M), ``recall`` (T, K, A, M), ``scores`` and the 12 ``stats``."""

    def __init__(self, params, ious, evalImgs, precision, recall, scores, stats):
        self.params, self.ious, self.evalImgs = params, ious, evalImgs
        self.precision, self.recall, self.scores, self.stats = precision, recall, scores, stats
        self.eval = {"params": params, "counts": list(precision.shape), "precision": precision, "recall": recall,
                     "scores": scores}


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


# -------------------------------------------------------------------------------------------------------------------
# host part: evaluateVid, accumulate, summarize
# -------------------------------------------------------------------------------------------------------------------
def _sorted_dets(dt, max_det):
    inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
    return [dt[i] for i in inds[0:max_det]]


def _evaluate_vid(p, gt, dt, ious_all, vidId, catId, aRng, maxDet):
    """``evaluateVid`` (:267-345) for the ground truths ``gt`` and detections ``dt`` of one (video, category)."""
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
    return {'video_id': vidId, 'category_id': catId, 'aRng': aRng, 'maxDet': maxDet,
            'dtIds': [d['id'] for d in dt], 'gtIds': [g['id'] for g in gt], 'dtMatches': dtm, 'gtMatches': gtm,
            'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}


def _accumulate(p, evalImgs):
    """``accumulate`` (:347-450) with the parameters the evaluation ran with."""
    T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
    precision = -np.ones((T, R, K, A, M))                             # -1 for absent settings (:366-368)
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    I0 = len(p.vidIds)
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


def evaluate_ytvis(gt, results, device=None, params=None, pred_bits=None, _counts=None) -> YTVISEvalResult:
    """gt: a :class:`YTVISGroundTruth`; results: the list ``instances_to_coco_json_video`` writes (``video_id``,
    ``score``, ``category_id``, ``segmentations`` with one RLE or ``None`` per frame); ``pred_bits`` optionally maps
    a video id to the (D, T, H, words) planes of that video's results, in their order, which are then not decoded.
    ``device`` is where the planes are built and counted (CPU by default).  Only ``iouType="segm"`` and
    ``useCats=1`` are supported.

    Reference behaviours reproduced (ytvoseval.py unless named):
      * detection ids are ``index + 1`` in the results list (ytvos.py:249) and ``iscrowd = 0`` (ytvos.py:255);
      * a detection's ``avg_area`` is the mean of its per-frame mask areas without the zero-area and missing frames,
        ``l = [a for a in ann['areas'] if a]`` (ytvos.py:250-254); a ground truth's comes from its ``areas`` field
        the same way (:100-104);
      * a ground truth is ignored when it is a crowd (:120) or its ``avg_area`` is outside the area range (:283);
      * detections are ordered by score and ground truths by ignore flag with the stable mergesort (:186, :289, :291);
      * detections beyond ``maxDets[-1]`` per (video, category) are dropped (:188-189, :292);
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
    Sequences of one video must have one length (the reference's ``zip`` would cut them to the shorter)."""
    p = copy.deepcopy(params) if params is not None else YTVISParams()
    if getattr(p, "iouType", "segm") != "segm" or getattr(p, "useSegm", None) is not None:
        raise NotImplementedError("only iouType='segm' is supported")
    if not p.useCats:
        raise NotImplementedError("only useCats=1 is supported")
    vid_ids = p.vidIds if len(p.vidIds) else sorted(gt.video_ids())
    cat_ids = p.catIds if len(p.catIds) else sorted(gt.category_ids())
    p.vidIds = list(np.unique(vid_ids))
    p.catIds = list(np.unique(cat_ids))
    p.maxDets = sorted(p.maxDets)
    maxDet = p.maxDets[-1]
    known = set(gt.video_ids())
    if any(r["video_id"] not in known for r in results):
        raise ValueError("results name videos the ground truth does not hold")      # ytvos.py:231
    cats = set(p.catIds)

    dets_of = {}
    for index, r in enumerate(results):
        if "segmentations" not in r:
            raise ValueError("results must hold 'segmentations'")
        dets_of.setdefault(r["video_id"], []).append((index, r))

    gts_by, dts_by, ious = {}, {}, {}
    for vidId in p.vidIds:
        anns = gt.vid_to_anns.get(vidId, [])
        dets = dets_of.get(vidId, [])
        if _counts is not None and vidId in _counts:
            inter, area_d, area_g = _counts[vidId]
        elif anns or dets:
            bits = pred_bits.get(vidId) if pred_bits else None
            inter, area_d, area_g = video_pair_counts(gt, vidId, [r for _, r in dets], device, bits)
        sum_g = area_g.sum(1) if anns else None
        for j, ann in enumerate(anns):
            if ann["category_id"] in cats:
                gts_by.setdefault((vidId, ann["category_id"]), []).append(
                    {"id": ann["id"], "row": j, "iscrowd": ann.get("iscrowd", 0),
                     "ignore": bool(ann.get("iscrowd", 0)), "avg_area": _avg_area(ann["areas"])})
        for i, (index, r) in enumerate(dets):
            if r["category_id"] in cats:
                areas = [int(a) if s else None for a, s in zip(area_d[i], r["segmentations"])]
                dts_by.setdefault((vidId, r["category_id"]), []).append(
                    {"id": index + 1, "row": i, "score": r["score"], "avg_area": _avg_area(areas)})
        for catId in p.catIds:
            g, d = gts_by.get((vidId, catId), []), dts_by.get((vidId, catId), [])
            if len(g) == 0 and len(d) == 0:
                ious[vidId, catId] = []
                continue
            d = _sorted_dets(d, maxDet)
            rows_d, rows_g = [x["row"] for x in d], [x["row"] for x in g]
            i = inter[np.ix_(rows_d, rows_g)].astype(np.float64)
            u = area_d[rows_d].sum(1)[:, None].astype(np.float64) + sum_g[rows_g][None, :] - i if rows_g else i
            out = np.zeros([len(d), len(g)])
            np.divide(i, u, out=out, where=u > .0)                    # 0 where the union is empty (:216)
            ious[vidId, catId] = out

    evalImgs = [_evaluate_vid(p, gts_by.get((vidId, catId), []), dts_by.get((vidId, catId), []), ious[vidId, catId],
                              vidId, catId, aRng, maxDet)
                for catId in p.catIds for aRng in p.areaRng for vidId in p.vidIds]
    precision, recall, scores = _accumulate(p, evalImgs)
    return YTVISEvalResult(p, ious, evalImgs, precision, recall, scores, _summarize(p, precision, recall))


# -------------------------------------------------------------------------------------------------------------------
# the evaluator
# -------------------------------------------------------------------------------------------------------------------
class YTVISEvaluator:
    """The reference's ``YTVISEvaluator`` (ytvis_eval.py:27-253) without detectron2: ``reset()``, ``process(inputs,
    outputs)`` per video and ``evaluate()``.

    ``process`` takes the dict of :class:`VideoMaskFormerInference` in any of its forms (bool, ``packed=True``,
    ``rle=True``).  When it holds ``"pred_bits"`` (``keep_bits=True``) the video's pair counts are taken at once from
    those planes, on their device, and only the counts are kept: the predictions are neither uploaded nor decoded
    again.  ``results`` is the accumulated ``results.json`` list (contiguous category ids, as the head wrote them)."""

    def __init__(self, ground_truth, thing_dataset_id_to_contiguous_id=None, class_names=None, device=None,
                 params=None):
        self.gt = ground_truth if isinstance(ground_truth, YTVISGroundTruth) else YTVISGroundTruth(ground_truth)
        self.id_map = thing_dataset_id_to_contiguous_id
        self.class_names = class_names
        self.device = device
        self.params = params
        self.reset()

    def reset(self):
        self._predictions = []
        self._counts = {}

    @property
    def results(self):
        return self._predictions

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
        metrics = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10"]
        stats = self.last.stats
        res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(metrics)}
        names = self.class_names
        if names is not None and len(names) > 1:
            precisions = self.last.precision
            assert len(names) == precisions.shape[2]
            for idx, name in enumerate(names):
                pr = precisions[:, :, idx, 0, -1]
                pr = pr[pr > -1]
                res["AP-" + "{}".format(name)] = float(np.mean(pr) * 100) if pr.size else float("nan")
        return {"segm": res}
