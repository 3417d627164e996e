"""Generate the Boundary AP fixtures (boundary_eval_gt.json, boundary_eval_results.json, boundary_eval_expected.npz)
from the seeded synthetic dataset of gen_coco_eval_golden.py, extended (nothing from the reference tree is copied).

    python tests/golden/gen_boundary_eval_golden.py --ref /path/to/reference

The oracle.  Neither ``boundary_iou`` nor ``cv2`` nor ``pycocotools`` is available, so the boundary-iou-api's
``COCOeval`` cannot be run.  As in gen_coco_eval_golden.py the matching, accumulation and summary are the reference's
``YTVOSeval`` on one-frame videos with COCO's area ranges, and ``computeIoU`` is replaced: here by the dense
``min(mask IoU, boundary IoU)`` with COCO's crowd rule on both, the boundaries eroded by
``scipy.ndimage.binary_erosion`` on dense masks (tests/boundary_ref.py).  It shares no code with bm2f_amd.  Parity
with the boundary-iou-api rests on this construction: nobody has run that package against this code.

The conditions the data must meet are asserted at the end (``check_coverage``): the run fails, and writes nothing,
rather than produce fixtures that miss one.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import boundary_ref  # noqa: E402
import gen_coco_eval_golden as base  # noqa: E402
from boundary_eval_cases import CONFIGS, EXPECTED_NPZ, GT_JSON, RESULTS_JSON  # noqa: E402
from coco_eval_cases import COCO_AREA_RNG, flatten  # noqa: E402
from gen_ytvis_eval_golden import _counts, _dense, encode_mask, import_reference  # noqa: E402


def build_dataset():
    """The COCO AP dataset plus three images for what only Boundary AP tells apart."""
    gt, results = base.build_dataset()
    sizes = {}

    def image(img, size):
        sizes[img] = size
        gt["images"].append({"id": img, "height": size[0], "width": size[1], "file_name": f"{img:012d}.jpg"})

    def add_gt(img, cat, mask, iscrowd=0, uncompressed=False):
        seg = {"size": list(mask.shape), "counts": _counts(mask)} if uncompressed else encode_mask(mask)
        gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": img, "category_id": cat,
                                  "iscrowd": iscrowd, "segmentation": seg, "area": float(mask.sum()),
                                  "bbox": base.bbox_of(mask)})

    def add_det(img, cat, score, mask):
        results.append({"image_id": img, "category_id": cat, "bbox": base.bbox_of(mask), "score": float(score),
                        "segmentation": encode_mask(mask)})

    # image 10, 1000 x 1300 (d = 33: the boundaries cross whole words).  Category 1: a detection 40 pixels inside
    # its ground truth all round, mask IoU 0.78 and disjoint boundaries; a second one that fits both ways.
    # Category 2: a crowd (uncompressed) and a detection in its corner that only the crowd rule on the boundary IoU
    # lifts over 0.5; category 3: an ellipse and a jittered copy
    s = (1000, 1300)
    image(10, s)
    add_gt(10, 1, base.rect(s, 100, 700, 100, 900))
    add_det(10, 1, 0.95, base.rect(s, 140, 660, 140, 860))
    add_gt(10, 1, base.rect(s, 750, 950, 100, 500))
    add_det(10, 1, 0.85, base.rect(s, 752, 950, 100, 497))
    add_gt(10, 2, base.rect(s, 700, 900, 900, 1200), iscrowd=1, uncompressed=True)
    add_det(10, 2, 0.9, base.rect(s, 700, 800, 900, 1000))
    add_gt(10, 3, base.ellipse(s, 300, 1100, 200, 150))
    add_det(10, 3, 0.7, base.ellipse(s, 306, 1096, 204, 150))

    # image 11, 300 x 420 (d = 10): thin objects, 12 rows and 9 columns, whose boundary is the whole mask
    t = (300, 420)
    image(11, t)
    add_gt(11, 2, base.rect(t, 50, 62, 40, 300))
    add_det(11, 2, 0.65, base.rect(t, 51, 62, 44, 300))
    add_gt(11, 1, base.rect(t, 100, 280, 350, 359))
    add_det(11, 1, 0.55, base.rect(t, 100, 270, 350, 359))
    # a blob that the erosion leaves a core of, with a detection that keeps the outline and loses the inside
    add_gt(11, 3, base.ellipse(t, 180, 150, 70, 90))
    add_det(11, 3, 0.6, base.ellipse(t, 180, 150, 70, 90) & ~base.ellipse(t, 180, 150, 35, 45))

    # image 12, 200 x 24 (narrower than a word, d = 4)
    u = (200, 24)
    image(12, u)
    add_gt(12, 1, base.rect(u, 20, 120, 2, 22))
    add_det(12, 1, 0.5, base.rect(u, 24, 120, 2, 21))
    return gt, results, sizes


def make_compute_iou(ev, ratio, sizes):
    """``computeIoU`` for the reference evaluator: ``ratio`` None is the mask IoU alone."""
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
                dm, gm = _dense(d["segmentations"][0]), _dense(g["segmentations"][0])
                if ratio is None:
                    ious[i, j] = base.dense_iou(dm, gm, bool(g["iscrowd"]))
                else:
                    ious[i, j] = boundary_ref.boundary_iou(dm, gm, boundary_ref.dilation(*sizes[vidId], ratio),
                                                           bool(g["iscrowd"]))
        return ious
    return compute


def run_reference(mods, gt, results, max_dets, ratio, sizes):
    import contextlib
    import io
    import tempfile
    ytvos, ytvoseval = mods
    vgt, vres = base.as_videos(gt, results, "segm")
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        path = os.path.join(tmp, "gt.json")
        with open(path, "w") as f:
            json.dump(vgt, f)
        g = ytvos.YTVOS(path)
        d = g.loadRes(vres)
        ev = ytvoseval.YTVOSeval(g, d)
        ev.params.iouType = "segm"
        ev.params.maxDets = list(max_dets)
        ev.params.areaRng = [list(r) for r in COCO_AREA_RNG]
        ev.computeIoU = make_compute_iou(ev, ratio, sizes)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return ev


def check_coverage(gt, results, evals, sizes):
    bd, wide, segm = evals["boundary"], evals["wide"], evals["segm"]
    ratio = CONFIGS["boundary"][2]
    d_of = {img: boundary_ref.dilation(*size, ratio) for img, size in sizes.items()}
    anns = gt["annotations"]
    pairs = [(r, a) for a in anns for r in results
             if (r["image_id"], r["category_id"]) == (a["image_id"], a["category_id"])]

    def ious(r, a, crowd):
        dm, gm, d = _dense(r["segmentation"]), _dense(a["segmentation"]), d_of[a["image_id"]]
        bdm, bgm = boundary_ref.boundary(dm, d), boundary_ref.boundary(gm, d)
        return (base.dense_iou(dm, gm, crowd), base.dense_iou(bdm, bgm, crowd))

    # mask IoU >= 0.5 > boundary IoU, and it changes a match
    assert any(m >= 0.5 > b for r, a in pairs if not a["iscrowd"] for m, b in [ious(r, a, False)]), "no such pair"
    match_b = flatten(bd.ious, bd.evalImgs, bd.eval["precision"], bd.eval["recall"], bd.eval["scores"], bd.stats, 10,
                      id_key="video_id")
    match_s = flatten(segm.ious, segm.evalImgs, segm.eval["precision"], segm.eval["recall"], segm.eval["scores"],
                      segm.stats, 10, id_key="video_id")
    assert not np.array_equal(match_b["dtMatches"], match_s["dtMatches"]), "no match changes against segm"
    assert bd.stats[0] > 0 and bd.stats[0] != segm.stats[0], "stats[0] must be positive and differ from segm"
    assert wide.stats[0] > 0 and not np.array_equal(wide.stats, bd.stats), "the second ratio changes nothing"
    # a thin object whose boundary is the whole mask
    assert any(m.any() and np.array_equal(boundary_ref.boundary(m, d_of[a["image_id"]]), m)
               for a in anns for m in [_dense(a["segmentation"])]), "no thin object"
    # the crowd rule acts on the boundary IoU
    assert any(ious(r, a, True)[1] >= 0.5 > ious(r, a, False)[1] for r, a in pairs if a["iscrowd"]), \
        "no crowd pair that only the crowd rule lifts over 0.5 on the boundary IoU"
    # an empty pair, union 0
    assert any(not _dense(r["segmentation"]).any() and not _dense(a["segmentation"]).any() for r, a in pairs), \
        "no pair with union 0"
    used = {a["image_id"] for a in anns} | {r["image_id"] for r in results}
    assert any(sizes[i][1] < 32 and d_of[i] == 1 for i in used), "no image narrower than 32 pixels with d = 1"
    assert any(d_of[i] >= 32 for i in used), "no image with d >= 32"
    assert any(isinstance(a["segmentation"]["counts"], list) for a in anns), "no uncompressed-RLE ground truth"
    assert CONFIGS["wide"][2] != 0.02
    assert max(boundary_ref.dilation(*s, CONFIGS["wide"][2]) for s in sizes.values()) <= 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    mods = import_reference(a.ref)
    gt, results, extra = build_dataset()
    sizes = {im["id"]: (im["height"], im["width"]) for im in gt["images"]}
    assert all(sizes[k] == v for k, v in extra.items())
    evals, arrays = {}, {}
    for name, (max_dets, _, ratio) in CONFIGS.items():
        ev = run_reference(mods, gt, results, max_dets, ratio, sizes)
        evals[name] = ev
        flat = flatten(ev.ious, ev.evalImgs, ev.eval["precision"], ev.eval["recall"], ev.eval["scores"], ev.stats,
                       len(ev.params.iouThrs), id_key="video_id")
        arrays.update({f"{name}/{k}": v for k, v in flat.items()})
    check_coverage(gt, results, evals, sizes)
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
