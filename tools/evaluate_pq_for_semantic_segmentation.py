#!/usr/bin/env python
"""PQ and mIoU of a semantic ``sem_seg_predictions.json``, in the role of the reference's
``tools/evaluate_pq_for_semantic_segmentation.py`` and without its dependencies (detectron2, panopticapi,
pycocotools):

    python tools/evaluate_pq_for_semantic_segmentation.py --json-file sem_seg_predictions.json --gt-dir DIR
        --num-classes K --ignore-label L [--gt-suffix .png] [--class-names FILE] [--device cuda]

The reference takes the class list, the ignore label and the ground-truth directory from detectron2's
``MetadataCatalog`` by ``--dataset-name``; here they are arguments.  ``category_id`` is taken as the contiguous class
id (what :func:`bm2f_amd.sem_seg_to_coco_json` writes without a mapping).  Every image named in the file is scored:
its ground truth is ``GT_DIR/<image id><suffix>`` read with PIL, its prediction a zero map painted with the file's
RLEs in file order on ``--device`` (``bm2f_amd.load_sem_seg_predictions``), and ``SemSegEvaluator(with_pq=True)``
counts both.  Prints the PQ / SQ / RQ / N table for All and Stuff (every class is stuff), then mIoU (a fraction, as
the reference prints it).  The reference tool itself has not been run against this one."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import SemSegEvaluator, load_sem_seg_predictions  # noqa: E402
from bm2f_amd.evaluation import sem_seg_image_id  # noqa: E402

BATCH = 16


def evaluate_predictions(predictions, ground_truths, num_classes, ignore_label, class_names=None, device=None):
    """predictions: the list of a ``sem_seg_predictions.json``; ground_truths: ``{image id: (H, W) integer array}``
    -> the :class:`SemSegEvaluator` (``with_pq=True``) after every image named by the predictions."""
    ids = list(dict.fromkeys(sem_seg_image_id(p["file_name"]) for p in predictions))
    ev = SemSegEvaluator(num_classes, ignore_label, class_names, device, with_pq=True)
    by_image = {i: [] for i in ids}
    for p in predictions:
        by_image[sem_seg_image_id(p["file_name"])].append(p)
    for k in range(0, len(ids), BATCH):
        batch = ids[k:k + BATCH]
        maps = load_sem_seg_predictions([p for i in batch for p in by_image[i]],
                                        {i: ground_truths[i].shape for i in batch}, device=device)
        ev.process([{"sem_seg": ground_truths[i], "image_id": i} for i in batch],
                   [{"sem_seg_labels": maps[i]} for i in batch])
    return ev


def report_lines(ev):
    """The PQ table and the mIoU line of an evaluator."""
    head = f"{'':<10}|" + "".join(f"{h:>7}" for h in ("PQ", "SQ", "RQ", "N"))
    lines = [head, "-" * len(head)]
    for name, isthing in (("All", None), ("Stuff", False)):
        avg, _ = ev.pq_stat.pq_average(ev.categories, isthing=isthing)
        cells = "".join(f"{100 * avg[k]:7.1f}" for k in ("pq", "sq", "rq"))
        lines.append(f"{name:<10}|{cells}{avg['n']:7d}")
    miou = ev.evaluate()["sem_seg"]["mIoU"] / 100
    return lines + ["", f"mIoU: {miou}"]


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json-file", required=True)
    parser.add_argument("--gt-dir", required=True)
    parser.add_argument("--gt-suffix", default=".png")
    parser.add_argument("--num-classes", type=int, required=True)
    parser.add_argument("--ignore-label", type=int, required=True)
    parser.add_argument("--class-names", default=None, help="a file with one class name per line")
    parser.add_argument("--device", default=None, help="where the predictions are painted and counted (default: cpu)")
    args = parser.parse_args(argv)
    from PIL import Image
    with open(args.json_file) as f:
        predictions = json.load(f)
    names = None
    if args.class_names:
        with open(args.class_names) as f:
            names = [line.strip() for line in f if line.strip()]
    gts = {}
    for i in dict.fromkeys(sem_seg_image_id(p["file_name"]) for p in predictions):
        with Image.open(os.path.join(args.gt_dir, i + args.gt_suffix)) as im:
            gts[i] = np.asarray(im)
    ev = evaluate_predictions(predictions, gts, args.num_classes, args.ignore_label, names, args.device)
    print("\n".join(report_lines(ev)))


if __name__ == "__main__":
    main()
