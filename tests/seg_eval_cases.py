"""The semantic mIoU / PQ fixtures shared by their generator and the tests (tests/golden/gen_seg_eval_golden.py)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAPS_NPZ = os.path.join(GOLDEN, "seg_eval_maps.npz")
EXPECTED_JSON = os.path.join(GOLDEN, "seg_eval_expected.json")
NUM_CLASSES = 8
IGNORE_LABEL = 255


def load_fixture():
    """-> (gts, preds, expected): uint8 label maps per image and the recorded reference statistics:
    ``expected["images"][i][str(category)] = [tp, fp, fn, iou]`` and ``expected["total"]`` their sum in image order."""
    with np.load(MAPS_NPZ, allow_pickle=False) as z:
        n = len(z.files) // 2
        gts = [z[f"gt_{i}"] for i in range(n)]
        preds = [z[f"pred_{i}"] for i in range(n)]
    with open(EXPECTED_JSON) as f:
        expected = json.load(f)
    assert expected["num_classes"] == NUM_CLASSES and expected["ignore_label"] == IGNORE_LABEL
    return gts, preds, expected


def stats_rows(stats, num_classes=NUM_CLASSES):
    """{category: {"tp", "fp", "fn", "iou"}} or {str(category): [tp, fp, fn, iou]} -> a list of [tp, fp, fn, iou] per
    class, zeros for a class without an entry."""
    out = []
    for c in range(num_classes):
        r = stats.get(c, stats.get(str(c)))
        if r is None:
            out.append([0, 0, 0, 0.0])
        elif isinstance(r, dict):
            out.append([r["tp"], r["fp"], r["fn"], r["iou"]])
        else:
            out.append(list(r))
    return out
