"""Generate the image AP fixtures (coco_eval_gt.json, coco_eval_results.json, coco_eval_expected.npz) from a seeded
synthetic COCO dataset (nothing from the reference tree is copied).

    python tests/golden/gen_coco_eval_golden.py --ref /path/to/reference

The oracle.  ``pycocotools`` is not available, so ``COCOeval`` itself cannot be run.  The reference ships a derivative
of it, ``YTVOS`` / ``YTVOSeval`` (mask2former_video/data_video/datasets/ytvis_api), whose ``evaluateVid``,
``accumulate`` and ``summarize`` are ``COCOeval``'s with ``image`` renamed ``video``.  The dataset is handed to it as
videos of length 1, with

  * ``params.areaRng`` set to COCO's ranges (all / small < 32^2 / medium / large >= 96^2),
  * each annotation's ``areas`` set to ``[annotation area]``, so that a ground truth's range comes from its ``area``
    field as in ``COCOeval``; a detection's comes from its mask area (``loadRes``) or, for boxes, is set to ``w * h``,
  * the IoU matrices supplied by this file: ``YTVOSeval.computeIoU`` does not apply COCO's crowd rule (the union
    with a crowd is the detection's area), so ``computeIoU`` is replaced by ``dense_ious`` / ``box_ious`` below, written
    out from dense numpy masks and from xywh boxes, with the reference's own ordering and ``maxDets[-1]`` cut.

So the matching, accumulation and summary in the fixtures are the reference's; the IoU in them is a dense definition
that shares no code with bm2f_amd.  Parity with ``COCOeval`` rests on this construction: nobody has run ``COCOeval``
itself against this code.

The dense stand-in for ``pycocotools.mask`` and the RLE reader and writer are those of gen_ytvis_eval_golden.py.
The branches the data must reach are asserted at the end (``check_coverage``): the run fails rather than writing
fixtures that miss one.
"""
import argparse
import contextlib
import inspect
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from coco_eval_cases import COCO_AREA_RNG, CONFIGS, EXPECTED_NPZ, GT_JSON, RESULTS_JSON, flatten  # noqa: E402
from gen_ytvis_eval_golden import _counts, _dense, encode_mask, import_reference  # noqa: E402


# -------------------------------------------------------------------------------------------------------------------
# the dataset
# -------------------------------------------------------------------------------------------------------------------
def rect(size, y0, y1, x0, x1):
    H, W = size
    m = np.zeros((H, W), dtype=bool)
    m[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = True
    return m


def ellipse(size, cy, cx, ry, rx):
    y, x = np.mgrid[:size[0], :size[1]]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def bbox_of(mask):
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


class Builder:
    def __init__(self):
        self.images, self.anns, self.results, self.sizes = [], [], [], {}

    def image(self, img, size):
        self.sizes[img] = size
        self.images.append({"id": img, "height": size[0], "width": size[1], "file_name": f"{img:012d}.jpg"})

    def gt(self, img, cat, mask, iscrowd=0, uncompressed=False, area=None):
        seg = {"size": list(mask.shape), "counts": _counts(mask)} if uncompressed else encode_mask(mask)
        self.anns.append({"id": len(self.anns) + 1, "image_id": img, "category_id": cat, "iscrowd": iscrowd,
                          "segmentation": seg, "area": float(mask.sum() if area is None else area),
                          "bbox": bbox_of(mask)})

    def det(self, img, cat, score, mask):
        self.results.append({"image_id": img, "category_id": cat, "bbox": bbox_of(mask), "score": float(score),
                             "segmentation": encode_mask(mask)})


def build_dataset():
    b = Builder()
    rng = np.random.RandomState(11)

    # image 1, category 1: a regular small ground truth and a large crowd (stored uncompressed, as COCO does) that
    # two detections match, one of them a small box inside it that only the crowd rule lifts over 0.5; the detection
    # on the regular one then meets the crowd (the break); a far detection stays unmatched
    s = (300, 420)
    b.image(1, s)
    b.gt(1, 1, rect(s, 20, 50, 30, 60))
    b.gt(1, 1, rect(s, 100, 260, 150, 330), iscrowd=1, uncompressed=True)
    b.det(1, 1, 0.9, rect(s, 22, 50, 30, 58))
    b.det(1, 1, 0.8, rect(s, 104, 260, 150, 326))
    b.det(1, 1, 0.8, rect(s, 110, 150, 160, 200))                     # equal score in one image
    b.det(1, 1, 0.3, rect(s, 270, 298, 380, 418))
    # category 2: a large ground truth; category 3: 900 pixels (small) whose area field says 2000 (medium)
    b.gt(1, 2, rect(s, 10, 290, 60, 330))
    b.det(1, 2, 0.7, rect(s, 14, 290, 60, 326))
    b.det(1, 2, 0.6, rect(s, 10, 150, 60, 330))
    b.gt(1, 3, rect(s, 200, 230, 350, 380), area=2000)
    b.det(1, 3, 0.75, rect(s, 200, 230, 352, 380))

    # image 2: ground truth and no detection; image 3 (narrower than 32): detections and no ground truth;
    # image 4: neither
    b.image(2, (200, 300))
    b.gt(2, 2, ellipse((200, 300), 100, 150, 40, 70))
    b.image(3, (64, 20))
    b.det(3, 3, 0.8, ellipse((64, 20), 30, 10, 12, 6))
    b.det(3, 1, 0.2, rect((64, 20), 2, 20, 1, 19))
    b.image(4, (50, 50))

    # image 5, category 1: seven detections, more than the reduced maxDets[-1] = 5, on a small, a medium and a large
    # ground truth; scores 0.9, 0.8, ...: equal to image 1's
    b.image(5, s)
    objs = [(40, 60, 15, 20), (150, 200, 35, 55), (230, 340, 50, 60)]
    for k, (cy, cx, ry, rx) in enumerate(objs):
        b.gt(5, 1, ellipse(s, cy, cx, ry, rx), uncompressed=k == 1)
    for n in range(7):
        cy, cx, ry, rx = objs[n % 3]
        dy, dx = rng.randint(-6, 7, size=2)
        b.det(5, 1, round(0.9 - 0.1 * n, 2), ellipse(s, cy + dy, cx + dx, ry + n, rx - n))

    # image 6 (40 x 31), category 2: intersection 1 of union 2, IoU exactly 0.5; category 3: an empty ground truth
    # against an empty detection, union 0
    t = (40, 31)
    b.image(6, t)
    two = np.zeros(t, dtype=bool)
    two[5, 7] = two[6, 7] = True
    one = np.zeros(t, dtype=bool)
    one[5, 7] = True
    b.gt(6, 2, two)
    b.det(6, 2, 0.5, one)
    b.gt(6, 3, np.zeros(t, dtype=bool))
    b.det(6, 3, 0.4, np.zeros(t, dtype=bool))

    # images 7-9: jittered copies of random objects in categories 1-3, with misses, false positives and crowds
    for img, size in ((7, (240, 320)), (8, (300, 420)), (9, (100, 150))):
        b.image(img, size)
        H, W = size
        for _ in range(rng.randint(2, 6)):
            cat = int(rng.randint(1, 4))
            ry, rx = rng.randint(4, H // 3), rng.randint(4, W // 3)
            cy, cx = rng.randint(ry, H - ry), rng.randint(rx, W - rx)
            b.gt(img, cat, ellipse(size, cy, cx, ry, rx), iscrowd=int(rng.rand() < 0.2),
                 uncompressed=bool(rng.rand() < 0.3))
            for _ in range(rng.randint(0, 3)):
                jy, jx = rng.randint(-ry // 3 - 1, ry // 3 + 2), rng.randint(-rx // 3 - 1, rx // 3 + 2)
                wrong = int(rng.randint(1, 4)) if rng.rand() < 0.2 else cat
                b.det(img, wrong, round(float(rng.rand()), 3), ellipse(size, cy + jy, cx + jx, ry + 1, rx))
    categories = [{"id": i, "name": n, "supercategory": "object"}
                  for i, n in enumerate(("person", "dog", "car", "kite"), start=1)]     # category 4 stays empty
    return {"images": b.images, "categories": categories, "annotations": b.anns,
            "info": {"description": "synthetic"}}, b.results


# -------------------------------------------------------------------------------------------------------------------
# the IoU handed to the reference, with COCO's crowd rule written out
# -------------------------------------------------------------------------------------------------------------------
def dense_iou(d, g, crowd):
    i = int((d & g).sum())
    u = int(d.sum()) if crowd else int((d | g).sum())
    return i / u if u > 0 else 0.0


def box_iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    i = max(w, 0.0) * max(h, 0.0)
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u if u > 0 else 0.0


def make_compute_iou(ev, iou_type):
    def compute(vidId, catId):
        p = ev.params
        gt, dt = ev._gts[vidId, catId], ev._dts[vidId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds][0:p.maxDets[-1]]
        ious = np.zeros([len(dt), len(gt)])
        for i, d in enumerate(dt):
            for j, g in enumerate(gt):
                if iou_type == "segm":
                    ious[i, j] = dense_iou(_dense(d["segmentations"][0]), _dense(g["segmentations"][0]),
                                           bool(g["iscrowd"]))
                else:
                    ious[i, j] = box_iou(d["bboxes"][0], g["bboxes"][0], bool(g["iscrowd"]))
        return ious
    return compute


def as_videos(gt, results, iou_type):
    """The COCO dicts as the one-frame YTVIS dicts the reference reads."""
    vgt = {"videos": [{"id": im["id"], "height": im["height"], "width": im["width"], "length": 1,
                       "file_names": [im["file_name"]]} for im in gt["images"]],
           "categories": gt["categories"], "info": gt["info"],
           "annotations": [{"id": a["id"], "video_id": a["image_id"], "category_id": a["category_id"],
                            "iscrowd": a["iscrowd"], "segmentations": [a["segmentation"]], "areas": [a["area"]],
                            "avg_area": a["area"], "bboxes": [a["bbox"]]} for a in gt["annotations"]]}
    vres = [{"video_id": r["image_id"], "score": r["score"], "category_id": r["category_id"],
             "segmentations": [r["segmentation"]], "bboxes": [list(r["bbox"])]} for r in results]
    return json.loads(json.dumps(vgt)), json.loads(json.dumps(vres))


def run_reference(mods, gt, results, max_dets, iou_type, trace_lines):
    ytvos, ytvoseval = mods
    code = ytvoseval.YTVOSeval.evaluateVid.__code__
    seen = set()

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(frame, event, arg):
            if event == "line" and frame.f_lineno in trace_lines:
                seen.add(frame.f_lineno)
            return local
        return local

    vgt, vres = as_videos(gt, results, iou_type)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        path = os.path.join(tmp, "gt.json")
        with open(path, "w") as f:
            json.dump(vgt, f)
        g = ytvos.YTVOS(path)
        d = g.loadRes(vres)
        if iou_type == "bbox":
            for ann in d.dataset["annotations"]:                      # COCO.loadRes: area = w * h for boxes
                ann["avg_area"] = ann["bboxes"][0][2] * ann["bboxes"][0][3]
        ev = ytvoseval.YTVOSeval(g, d)
        ev.params.iouType = iou_type
        ev.params.maxDets = list(max_dets)
        ev.params.areaRng = [list(r) for r in COCO_AREA_RNG]
        ev.computeIoU = make_compute_iou(ev, iou_type)
        sys.settrace(tracer)
        try:
            ev.evaluate()
        finally:
            sys.settrace(None)
        ev.accumulate()
        ev.summarize()
    return ev, seen


def area_range(a):
    return "small" if a < 32 ** 2 else "medium" if a < 96 ** 2 else "large"


def check_coverage(gt, results, evals, seen, break_line):
    """Every branch the fixtures are meant to reach is reached by the committed data."""
    ev, red = evals["default"], evals["reduced"]
    imgs = [e for e in ev.evalImgs if e is not None]
    anns = gt["annotations"]
    crowd_ids = {a["id"] for a in anns if a["iscrowd"]}
    sizes = {(im["height"], im["width"]) for im in gt["images"]}
    assert len(sizes) >= 3 and any(w % 32 for _, w in sizes) and any(w < 32 for _, w in sizes), "image sizes"
    assert any(sum(1 for g in e["dtMatches"][0] if g in crowd_ids) >= 2 for e in imgs), "crowd matched twice"
    lifted = False
    for a in anns:
        if a["iscrowd"]:
            g = _dense(a["segmentation"])
            for r in results:
                if (r["image_id"], r["category_id"]) == (a["image_id"], a["category_id"]):
                    d = _dense(r["segmentation"])
                    lifted |= dense_iou(d, g, False) < 0.5 <= dense_iou(d, g, True)
    assert lifted, "a detection only the crowd rule lifts over 0.5"
    assert break_line in seen, "the break on ignore never fired"
    assert any(area_range(a["area"]) != area_range(int(_dense(a["segmentation"]).sum())) for a in anns), \
        "an area field in another range than the mask area"
    assert any(e["gtIgnore"][i] and gid not in crowd_ids for e in imgs for i, gid in enumerate(e["gtIds"])), \
        "ground truth ignored by area range"
    assert any(e["gtIgnore"][i] and gid in crowd_ids for e in imgs for i, gid in enumerate(e["gtIds"])), \
        "ground truth ignored as crowd"
    assert any(((e["dtMatches"] == 0) & e["dtIgnore"]).any() for e in imgs), "unmatched detection outside the range"
    assert any(((e["dtMatches"] > 0) & e["dtIgnore"]).any() for e in imgs), "detection matched to an ignored gt"
    gt_imgs, dt_imgs = {a["image_id"] for a in anns}, {r["image_id"] for r in results}
    all_imgs = {im["id"] for im in gt["images"]}
    assert gt_imgs - dt_imgs, "an image with ground truth and no detections"
    assert dt_imgs - gt_imgs, "an image with detections and no ground truth"
    assert all_imgs - gt_imgs - dt_imgs, "an image with neither"
    used = {a["category_id"] for a in anns} | {r["category_id"] for r in results}
    absent = [k for k, c in enumerate(sorted(x["id"] for x in gt["categories"])) if c not in used]
    assert absent and (ev.eval["precision"][:, :, absent] == -1).all(), "a category absent everywhere"
    per_key = {}
    for r in results:
        per_key.setdefault((r["image_id"], r["category_id"]), []).append(r["score"])
    limit = CONFIGS["reduced"][0][-1]
    assert any(len(s) > limit for s in per_key.values()), "more detections than the reduced maxDets[-1]"
    assert all(len(e["dtIds"]) <= limit for e in red.evalImgs if e is not None)
    assert any(len(s) != len(set(s)) for s in per_key.values()), "equal scores in one image"
    by_cat = {}
    for (v, c), s in per_key.items():
        for x in s:
            by_cat.setdefault((c, x), set()).add(v)
    assert any(len(v) > 1 for v in by_cat.values()), "equal scores across images"
    halves = [(k, v) for k, v in ev.ious.items() if len(v) and (np.asarray(v) == 0.5).any()]
    assert halves, "an IoU exactly at a threshold"
    whole = [e for e in imgs if e["aRng"][0] == 0 and e["aRng"][1] > 1e9
             and any((e["video_id"], e["category_id"]) == k and np.asarray(v).shape == (1, 1) for k, v in halves)]
    assert whole and whole[0]["dtMatches"][0].any() and not whole[0]["dtMatches"][1].any(), \
        "IoU 0.5 matches at 0.5 only"
    empty_gt = [a for a in anns if _dense(a["segmentation"]).sum() == 0]
    empty_dt = [r for r in results if _dense(r["segmentation"]).sum() == 0]
    assert empty_dt, "an empty detection mask"
    assert any((r["image_id"], r["category_id"]) == (a["image_id"], a["category_id"])
               for a in empty_gt for r in empty_dt), "a pair with union 0"
    assert any(isinstance(a["segmentation"]["counts"], list) for a in anns), "an uncompressed-RLE ground truth"
    for name in ("small", "medium", "large"):
        i = ev.params.areaRngLbl.index(name)
        assert (ev.eval["recall"][:, :, i, -1] > -1).any(), f"no ground truth in the {name} range"
        assert any(area_range(a["area"]) == name and not a["iscrowd"] for a in anns), name
    assert ev.stats[0] > 0 and evals["bbox"].stats[0] > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    mods = import_reference(a.ref)
    gt, results = build_dataset()
    src, first = inspect.getsourcelines(mods[1].YTVOSeval.evaluateVid)
    break_line = first + next(i for i, line in enumerate(src) if line.strip() == "break")
    evals, arrays, seen = {}, {}, set()
    for name, (max_dets, iou_type) in CONFIGS.items():
        ev, s = run_reference(mods, gt, results, max_dets, iou_type, {break_line})
        if iou_type == "segm":
            seen |= s
        evals[name] = ev
        flat = flatten(ev.ious, ev.evalImgs, ev.eval["precision"], ev.eval["recall"], ev.eval["scores"], ev.stats,
                       len(ev.params.iouThrs), id_key="video_id")
        arrays.update({f"{name}/{k}": v for k, v in flat.items()})
    check_coverage(gt, results, evals, seen, break_line)
    with open(GT_JSON, "w") as f:
        json.dump(gt, f, separators=(",", ":"))
    with open(RESULTS_JSON, "w") as f:
        json.dump(results, f, separators=(",", ":"))
    np.savez_compressed(EXPECTED_NPZ, **arrays)
    for p in (GT_JSON, RESULTS_JSON, EXPECTED_NPZ):
        print(p, os.path.getsize(p), "bytes")
    print("stats", {k: np.round(v.stats, 4).tolist() for k, v in evals.items()})


if __name__ == "__main__":
    main()
