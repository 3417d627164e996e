"""Shared by tests/golden/gen_ytvis_eval_golden.py and the ytvis_eval tests: the two parameter sets the fixtures were
made with and the flat form in which an evaluation (the reference's ``YTVOSeval`` or ours) is stored and compared."""
import json
import os

import numpy as np

from coco_eval_cases import flatten as _flatten

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GT_JSON = os.path.join(GOLDEN, "ytvis_eval_gt.json")
RESULTS_JSON = os.path.join(GOLDEN, "ytvis_eval_results.json")
EXPECTED_NPZ = os.path.join(GOLDEN, "ytvis_eval_expected.npz")

# name -> maxDets; "reduced" makes 7 detections of one (video, category) exceed maxDets[-1]
CONFIGS = {"default": [1, 10, 100], "reduced": [1, 2, 5]}

FIELDS = ("iou_keys", "iou_shapes", "iou_values", "img_none", "img_meta", "img_nd", "img_ng", "dtIds", "gtIds",
          "dtMatches", "gtMatches", "dtScores", "gtIgnore", "dtIgnore", "precision", "recall", "scores", "stats")


def flatten(ious, eval_imgs, precision, recall, scores, stats, num_thresholds):
    """-> {field: array}; every field of every evalImgs record is kept, concatenated over the records."""
    return _flatten(ious, eval_imgs, precision, recall, scores, stats, num_thresholds, id_key="video_id")


def load_fixture():
    with open(GT_JSON) as f:
        gt = json.load(f)
    with open(RESULTS_JSON) as f:
        results = json.load(f)
    z = np.load(EXPECTED_NPZ)
    expected = {name: {f: z[f"{name}/{f}"] for f in FIELDS} for name in CONFIGS}
    return gt, results, expected
