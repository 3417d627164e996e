"""Generate the semantic PQ fixtures (seg_eval_maps.npz, seg_eval_expected.json) by running the reference's own
``pq_compute_single_image`` (tools/evaluate_pq_for_semantic_segmentation.py) on seeded synthetic (ground truth,
prediction) label maps.  Nothing from the reference tree is copied: only the maps and the recorded counters are
written.

    python tests/golden/gen_seg_eval_golden.py --ref /path/to/reference

The tool imports ``detectron2``, ``tqdm``, ``pycocotools`` and ``panopticapi.evaluation``; none is a dependency here,
so empty stand-ins are installed before the import (the function under test uses none of them but ``PQStat``).  The
``PQStat`` given to it is written below: four counters per category and ``+=``.

The prediction maps hold no ``ignore_label`` pixel (the reference function would raise on one).  The branches the data
must reach are asserted before anything is written (``check_coverage``), from a dense per-pixel count made here.
"""
import argparse
import importlib.util
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from seg_eval_cases import EXPECTED_JSON, IGNORE_LABEL, MAPS_NPZ, NUM_CLASSES  # noqa: E402


class PQStatCat:
    def __init__(self):
        self.iou = 0.0
        self.tp = 0
        self.fp = 0
        self.fn = 0

    def __iadd__(self, other):
        self.iou += other.iou
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        return self


class PQStat:
    def __init__(self):
        self.pq_per_cat = defaultdict(PQStatCat)

    def __getitem__(self, i):
        return self.pq_per_cat[i]

    def __iadd__(self, other):
        for label, cat in other.pq_per_cat.items():
            self.pq_per_cat[label] += cat
        return self

    def rows(self):
        return {str(int(c)): [int(s.tp), int(s.fp), int(s.fn), float(s.iou)] for c, s in sorted(self.pq_per_cat.items())}


def import_reference(ref_root):
    def stub(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    stub("tqdm", tqdm=lambda x, *a, **k: x)
    stub("detectron2")
    stub("detectron2.data", MetadataCatalog=None)
    stub("detectron2.data.detection_utils", read_image=None)
    stub("detectron2.utils")
    stub("detectron2.utils.file_io", PathManager=None)
    stub("pycocotools", mask=types.ModuleType("pycocotools.mask"))
    stub("pycocotools.mask")
    stub("panopticapi")
    stub("panopticapi.evaluation", PQStat=PQStat)
    path = os.path.join(ref_root, "tools", "evaluate_pq_for_semantic_segmentation.py")
    spec = importlib.util.spec_from_file_location("reference_pq_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# -------------------------------------------------------------------------------------------------------------------
# the label maps
# -------------------------------------------------------------------------------------------------------------------
def hand_made():
    """48 x 64: every branch the issue lists, by construction."""
    gt = np.zeros((48, 64), dtype=np.uint8)
    gt[4:24, 4:24] = 1
    gt[30:40, 10:50] = 2
    gt[:, 56:] = IGNORE_LABEL
    pred = np.zeros((48, 64), dtype=np.uint8)
    pred[4:24, 14:40] = 1            # 200 of its 520 pixels on the 400 of class 1: IoU 0.28, a rejected pair, fn and fp
    pred[30:40, 10:32] = 2           # 220 pixels inside the 400 of class 2: IoU 0.55
    pred[10:20, 54:64] = 3           # 80 of 100 pixels on VOID: an unmatched prediction spared; class 3 has no gt
    pred[42:46, 2:8] = 4             # on the background: a counted fp of a class absent from the ground truth
    return gt, pred


def random_pair(rng, h, w):
    gt = np.full((h, w), int(rng.randint(0, NUM_CLASSES)), dtype=np.uint8)
    pred = gt.copy()
    for _ in range(int(rng.randint(3, 7))):
        c = int(rng.randint(0, NUM_CLASSES))
        y0, x0 = int(rng.randint(0, max(h - 2, 1))), int(rng.randint(0, max(w - 2, 1)))
        y1, x1 = int(rng.randint(y0 + 1, h + 1)), int(rng.randint(x0 + 1, w + 1))
        gt[y0:y1, x0:x1] = c
        dy, dx = (int(v) for v in rng.randint(-4, 5, size=2))
        wrong = int(rng.randint(0, NUM_CLASSES)) if rng.rand() < 0.25 else c
        pred[max(y0 + dy, 0):max(y1 + dy, 0), max(x0 + dx, 0):max(x1 + dx, 0)] = wrong
    if rng.rand() < 0.7:
        y0, x0 = int(rng.randint(0, max(h - 2, 1))), int(rng.randint(0, max(w - 2, 1)))
        gt[y0:y0 + int(rng.randint(1, 9)), x0:x0 + int(rng.randint(1, 9))] = IGNORE_LABEL
    return gt, pred


def build_maps():
    rng = np.random.RandomState(11)
    pairs = [hand_made()]
    for h, w in ((48, 64), (17, 23), (31, 40), (1, 64), (33, 7)):
        pairs.append(random_pair(rng, h, w))
    return pairs


def check_coverage(pairs, stats):
    """The branches the issue lists are reached; from dense masks, independent of the function under test."""
    seen = set()
    for (gt, pred), st in zip(pairs, stats):
        assert not (pred == IGNORE_LABEL).any() and pred.max() < NUM_CLASSES, "a prediction holds the ignore label"
        assert gt.shape == pred.shape and gt.shape[0] <= 48 and gt.shape[1] <= 64
        assert ((gt < NUM_CLASSES) | (gt == IGNORE_LABEL)).all()
        tp_seen = set()
        for c in range(NUM_CLASSES):
            g, p = gt == c, pred == c
            if g.any() and p.any() and (g & p).any():
                iou = (g & p).sum() / (p.sum() + g.sum() - (g & p).sum() - (p & (gt == IGNORE_LABEL)).sum())
                if 0.5 < iou < 0.6:
                    seen.add("tp in (0.5, 0.6)")
                if iou <= 0.5:
                    seen.add("rejected pair")
                if iou > 0.5:
                    tp_seen.add(c)
            if p.any() and c not in tp_seen:
                frac = (p & (gt == IGNORE_LABEL)).sum() / p.sum()
                seen.add("fp spared by VOID" if frac > 0.5 else "fp counted")
                if frac > 0.5:
                    assert st.get(str(c), [0, 0, 0, 0.0])[1] == 0
            if g.any() and c not in tp_seen:
                seen.add("fn")
            if p.any() and not g.any():
                seen.add("class predicted but absent from the ground truth")
        assert {int(c) for c, r in st.items() if r[0]} == tp_seen, "the dense count disagrees on the matches"
    want = {"tp in (0.5, 0.6)", "rejected pair", "fp spared by VOID", "fp counted", "fn",
            "class predicted but absent from the ground truth"}
    assert seen >= want, f"not reached: {sorted(want - seen)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    tool = import_reference(a.ref)
    categories = {i: {"id": i, "name": str(i), "isthing": 0} for i in range(NUM_CLASSES)}
    pairs = build_maps()
    total, per_image = PQStat(), []
    for gt, pred in pairs:
        # the tool reads its ground truth as int64 (main(), astype(np.int64)) and builds the prediction zeros_like it
        single = tool.pq_compute_single_image(gt.astype(np.int64), pred.astype(np.int64), categories, IGNORE_LABEL)
        per_image.append(single.rows())
        total += single
    check_coverage(pairs, per_image)
    np.savez_compressed(MAPS_NPZ, **{f"gt_{i}": g for i, (g, _) in enumerate(pairs)},
                        **{f"pred_{i}": p for i, (_, p) in enumerate(pairs)})
    with open(EXPECTED_JSON, "w") as f:
        json.dump({"num_classes": NUM_CLASSES, "ignore_label": IGNORE_LABEL, "images": per_image,
                   "total": total.rows()}, f, indent=1)
    for p in (MAPS_NPZ, EXPECTED_JSON):
        print(p, os.path.getsize(p), "bytes")
    print("total", total.rows())


if __name__ == "__main__":
    main()
