"""Shared by tests/golden/gen_boundary_eval_golden.py and the boundary tests: the parameter sets the Boundary AP
fixtures were made with.  The flat form of an evaluation is ``coco_eval_cases.flatten``."""
import json
import os

import numpy as np

from coco_eval_cases import FIELDS, GOLDEN

GT_JSON = os.path.join(GOLDEN, "boundary_eval_gt.json")
RESULTS_JSON = os.path.join(GOLDEN, "boundary_eval_results.json")
EXPECTED_NPZ = os.path.join(GOLDEN, "boundary_eval_expected.npz")

# name -> (maxDets, iou type, dilation ratio); "segm" is the same data under mask IoU alone, which the boundary
# results must differ from
CONFIGS = {"boundary": ([1, 10, 100], "boundary", 0.02), "wide": ([1, 10, 100], "boundary", 0.05),
           "segm": ([1, 10, 100], "segm", None)}


def load_fixture():
    with open(GT_JSON) as f:
        gt = json.load(f)
    with open(RESULTS_JSON) as f:
        results = json.load(f)
    z = np.load(EXPECTED_NPZ)
    expected = {name: {f: z[f"{name}/{f}"] for f in FIELDS} for name in CONFIGS}
    return gt, results, expected
