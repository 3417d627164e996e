"""A dense per-pixel restatement of the PQ matching rules (the issue's section 4), for tests: it loops over segments
with boolean masks, never forms a table of counts and shares no code with bm2f_amd.

    pq_single(gt_map, gt_segments, pred_map, pred_segments, categories, void=0) -> {category: [tp, fp, fn, iou]}
    pq_total(per_image) -> the sum, category by category, in image order
    pq_average(total, categories, isthing=None) -> (pq, sq, rq, n)

gt_segments: dicts with id, category_id, iscrowd; pred_segments: dicts with id, category_id; categories: {id:
{"isthing": 0 / 1}}.  Pairs are visited in ascending (ground-truth id, predicted id) order."""
import numpy as np


def pq_single(gt_map, gt_segments, pred_map, pred_segments, categories, void=0, pred_void=0, image_id=None):
    gt_map, pred_map = np.asarray(gt_map).astype(np.int64), np.asarray(pred_map).astype(np.int64)
    stats = {c: [0, 0, 0, 0.0] for c in categories}
    void_mask = gt_map == void
    listed = {s["id"]: s for s in pred_segments}
    for label in np.unique(pred_map).tolist():
        if label not in listed:
            if pred_void is not None and label == pred_void:
                continue
            raise KeyError("In the image with ID {} segment with ID {} is presented in PNG and not presented in "
                           "JSON.".format(image_id, label))
        if listed[label]["category_id"] not in categories:
            raise KeyError("In the image with ID {} segment with ID {} has unknown category_id {}.".format(
                image_id, label, listed[label]["category_id"]))
    absent = [p for p in listed if not (pred_map == p).any()]
    if absent:
        raise KeyError("In the image with ID {} the following segment IDs {} are presented in JSON and not presented "
                       "in PNG.".format(image_id, absent))

    gt_matched, pred_matched = set(), set()
    for g in sorted(gt_segments, key=lambda s: s["id"]):
        if g.get("iscrowd", 0) == 1:
            continue
        g_mask = gt_map == g["id"]
        for p in sorted(pred_segments, key=lambda s: s["id"]):
            if p["category_id"] != g["category_id"]:
                continue
            p_mask = pred_map == p["id"]
            inter = int((g_mask & p_mask).sum())
            if inter == 0:
                continue
            union = int(p_mask.sum()) + int(g_mask.sum()) - inter - int((void_mask & p_mask).sum())
            iou = np.float64(inter) / np.float64(union)
            if iou > 0.5:
                stats[g["category_id"]][0] += 1
                stats[g["category_id"]][3] += iou
                gt_matched.add(g["id"])
                pred_matched.add(p["id"])
    crowd = {}
    for g in gt_segments:
        if g["id"] in gt_matched:
            continue
        if g.get("iscrowd", 0) == 1:
            crowd[g["category_id"]] = g["id"]
            continue
        stats[g["category_id"]][2] += 1
    for p in pred_segments:
        if p["id"] in pred_matched:
            continue
        p_mask = pred_map == p["id"]
        spared = int((void_mask & p_mask).sum())
        if p["category_id"] in crowd:
            spared += int(((gt_map == crowd[p["category_id"]]) & p_mask).sum())
        if np.float64(spared) / np.float64(p_mask.sum()) > 0.5:
            continue
        stats[p["category_id"]][1] += 1
    return stats


def pq_total(per_image):
    total = None
    for st in per_image:
        if total is None:
            total = {c: [0, 0, 0, 0.0] for c in st}
        for c, r in st.items():
            for k in range(4):
                total[c][k] += r[k]
    return total


def pq_average(total, categories, isthing=None):
    pq = sq = rq = 0.0
    n = 0
    for c, info in categories.items():
        if isthing is not None and bool(info["isthing"]) != isthing:
            continue
        tp, fp, fn, iou = total[c]
        if tp + fp + fn == 0:
            continue
        n += 1
        pq += iou / (tp + 0.5 * fp + 0.5 * fn)
        sq += iou / tp if tp else 0.0
        rq += tp / (tp + 0.5 * fp + 0.5 * fn)
    if n == 0:
        return float("nan"), float("nan"), float("nan"), 0
    return pq / n, sq / n, rq / n, n
