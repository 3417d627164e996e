"""Shared by tests/golden/gen_coco_eval_golden.py and the coco_eval tests: the parameter sets the fixtures were made
with and the flat form in which an evaluation (the oracle's or ours) is stored and compared."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GT_JSON = os.path.join(GOLDEN, "coco_eval_gt.json")
RESULTS_JSON = os.path.join(GOLDEN, "coco_eval_results.json")
EXPECTED_NPZ = os.path.join(GOLDEN, "coco_eval_expected.npz")

# name -> (maxDets, iou type); "reduced" makes 7 detections of one (image, category) exceed maxDets[-1]
CONFIGS = {"default": ([1, 10, 100], "segm"), "reduced": ([1, 2, 5], "segm"), "bbox": ([1, 10, 100], "bbox")}

COCO_AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]

FIELDS = ("iou_keys", "iou_shapes", "iou_values", "img_none", "img_meta", "img_nd", "img_ng", "dtIds", "gtIds",
          "dtMatches", "gtMatches", "dtScores", "gtIgnore", "dtIgnore", "precision", "recall", "scores", "stats")


def flatten(ious, eval_imgs, precision, recall, scores, stats, num_thresholds, id_key="image_id"):
    """-> {field: array}; every field of every evalImgs record is kept, concatenated over the records.  ``id_key``
    names the image of a record (the oracle, run on one-frame videos, says ``video_id``)."""
    keys = sorted(ious.keys())
    shapes, values = [], []
    for k in keys:
        v = ious[k]
        if isinstance(v, list) and len(v) == 0:
            shapes.append((-1, -1))                                   # [] for a pair without anything
        else:
            v = np.asarray(v, dtype=np.float64)
            shapes.append(v.shape)
            values.append(v.reshape(-1))
    live = [e for e in eval_imgs if e is not None]
    T = num_thresholds

    def cat(field, axis, empty):
        parts = [np.asarray(e[field], dtype=np.float64) for e in live]
        return np.concatenate(parts, axis=axis) if parts else empty

    return {
        "iou_keys": np.asarray(keys, dtype=np.int64).reshape(-1, 2),
        "iou_shapes": np.asarray(shapes, dtype=np.int64).reshape(-1, 2),
        "iou_values": np.concatenate(values) if values else np.zeros(0),
        "img_none": np.asarray([e is None for e in eval_imgs]),
        "img_meta": np.asarray([[e[id_key], e["category_id"], e["aRng"][0], e["aRng"][1], e["maxDet"]]
                                for e in live], dtype=np.float64).reshape(-1, 5),
        "img_nd": np.asarray([len(e["dtIds"]) for e in live], dtype=np.int64),
        "img_ng": np.asarray([len(e["gtIds"]) for e in live], dtype=np.int64),
        "dtIds": cat("dtIds", 0, np.zeros(0)),
        "gtIds": cat("gtIds", 0, np.zeros(0)),
        "dtMatches": cat("dtMatches", 1, np.zeros((T, 0))),
        "gtMatches": cat("gtMatches", 1, np.zeros((T, 0))),
        "dtScores": cat("dtScores", 0, np.zeros(0)),
        "gtIgnore": cat("gtIgnore", 0, np.zeros(0)),
        "dtIgnore": cat("dtIgnore", 1, np.zeros((T, 0))),
        "precision": np.asarray(precision), "recall": np.asarray(recall), "scores": np.asarray(scores),
        "stats": np.asarray(stats, dtype=np.float64),
    }


def load_fixture():
    with open(GT_JSON) as f:
        gt = json.load(f)
    with open(RESULTS_JSON) as f:
        results = json.load(f)
    z = np.load(EXPECTED_NPZ)
    expected = {name: {f: z[f"{name}/{f}"] for f in FIELDS} for name in CONFIGS}
    return gt, results, expected
