#!/usr/bin/env python
"""COCO Boundary AP (or mask AP) of a results file, with the arguments of the reference's
``tools/evaluate_coco_boundary_ap.py`` and without its dependencies (``boundary_iou``, OpenCV, pycocotools):

    python tools/evaluate_coco_boundary_ap.py --gt-json-file COCO_GT_JSON --dt-json-file COCO_DT_JSON
                                              [--iou-type boundary|segm] [--dilation-ratio 0.02]
                                              [--device cuda] [--polygons refuse|rasterize]

Boundary IoU is ``min(mask IoU, IoU of the masks' boundaries)`` with the boundaries ``mask & ~erode(mask, d)`` and
``d = max(1, round(dilation_ratio * image diagonal))`` (``bm2f_amd.mask_boundary`` restates the definition; the
boundary-iou-api itself has not been run against it).  ``bbox`` fields of the results are dropped, as the reference
tool drops them.  Ground-truth polygons are refused unless ``--polygons rasterize`` (see ``bm2f_amd.coco_eval``).
Prints the 12-line summary of ``COCOeval.summarize``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import COCOGroundTruth, evaluate_coco  # noqa: E402


def summary_lines(result):
    p, stats = result.params, result.stats
    rows = [(1, None, "all", 100), (1, .5, "all", p.maxDets[2]), (1, .75, "all", p.maxDets[2]),
            (1, None, "small", p.maxDets[2]), (1, None, "medium", p.maxDets[2]), (1, None, "large", p.maxDets[2]),
            (0, None, "all", p.maxDets[0]), (0, None, "all", p.maxDets[1]), (0, None, "all", p.maxDets[2]),
            (0, None, "small", p.maxDets[2]), (0, None, "medium", p.maxDets[2]), (0, None, "large", p.maxDets[2])]
    out = []
    for (ap, thr, area, max_dets), value in zip(rows, stats):
        title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        iou = f"{p.iouThrs[0]:0.2f}:{p.iouThrs[-1]:0.2f}" if thr is None else f"{thr:0.2f}"
        out.append(f" {title:<18} {kind} @[ IoU={iou:<9} | area={area:>6s} | maxDets={max_dets:>3d} ] = {value:0.3f}")
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--gt-json-file", default="")
    parser.add_argument("--dt-json-file", default="")
    parser.add_argument("--iou-type", default="boundary", choices=("boundary", "segm"))
    parser.add_argument("--dilation-ratio", default=0.020, type=float)
    parser.add_argument("--device", default=None, help="where the masks are built and counted (default: cpu)")
    parser.add_argument("--polygons", default="refuse", choices=("refuse", "rasterize"))
    args = parser.parse_args(argv)
    print(args)
    with open(args.dt_json_file) as f:
        results = json.load(f)
    for r in results:                                                 # remove box predictions
        r.pop("bbox", None)
    gt = COCOGroundTruth(args.gt_json_file, polygons=args.polygons)
    result = evaluate_coco(gt, results, iou_type=args.iou_type, device=args.device,
                           dilation_ratio=args.dilation_ratio)
    print("\n".join(summary_lines(result)))
    return result.stats


if __name__ == "__main__":
    main()
