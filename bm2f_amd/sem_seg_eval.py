"""Semantic segmentation metrics without detectron2: the role of detectron2's ``SemSegEvaluator`` (metrics only; the
reference's ``train_net.py:build_evaluator`` attaches it to every ``sem_seg`` dataset) and of the reference's
``tools/evaluate_pq_for_semantic_segmentation.py``, which scores semantic predictions with PQ.

detectron2 copies every prediction to the host and adds ``np.bincount((K + 1) * pred + gt)`` to a confusion matrix.
Here a batch of images is one launch of the label-pair counting kernel (:mod:`bm2f_amd.label_counts`, direct mode,
``rows = cols = K + 1``, the ignore label in the last row) on the device the predictions already lie on, and only the
(K + 1) x (K + 1) integers reach the host.

With ``tp`` the diagonal of the K x K part of ``conf_matrix`` (detectron2's orientation, ``[pred, gt]``), ``pos_gt`` and
``pos_pred`` its column and row sums, ``acc_valid = pos_gt > 0``, ``iou_valid = pos_gt + pos_pred > 0`` and ``union =
pos_gt + pos_pred - tp``, all in fp64:

    acc = tp / pos_gt and iou = tp / union on acc_valid
    mIoU = sum(iou[acc_valid]) / sum(iou_valid)         mACC  = sum(acc[acc_valid]) / sum(acc_valid)
    fwIoU = sum(iou[acc_valid] * (pos_gt / sum(pos_gt))[acc_valid])       pACC = sum(tp) / sum(pos_gt)

With ``with_pq`` every image keeps its own table and also feeds :func:`bm2f_amd.panoptic_eval.pq_from_counts` as the
reference tool's ``pq_compute_single_image`` does: a segment is a class present in the image, its id is its category,
VOID is the ignore row, no segment is a crowd and every class is stuff.  detectron2's ``SemSegEvaluator`` itself has
not been run against this module.
"""
from __future__ import annotations

import numpy as np
import torch

from .label_counts import label_pair_counts_ragged
from .label_planes import as_label_plane, same_dtype
from .panoptic_eval import PQStat, pq_from_counts


def sem_seg_metrics(conf_matrix, class_names=None):
    """conf_matrix (K + 1, K + 1) int64 ``[pred, gt]`` -> the dict of mIoU, fwIoU, mACC, pACC, IoU-<name> and
    ACC-<name>, x 100 (detectron2's ``SemSegEvaluator.evaluate``; the mIoU lines are those of the reference tool)."""
    conf_matrix = np.asarray(conf_matrix, dtype=np.int64)
    K = conf_matrix.shape[0] - 1
    names = list(class_names) if class_names is not None else [str(k) for k in range(K)]
    if len(names) != K:
        raise ValueError(f"{len(names)} class names for {K} classes")
    acc = np.full(K, np.nan, dtype=np.float64)
    iou = np.full(K, np.nan, dtype=np.float64)
    tp = conf_matrix.diagonal()[:-1].astype(np.float64)
    pos_gt = np.sum(conf_matrix[:-1, :-1], axis=0).astype(np.float64)
    class_weights = pos_gt / np.sum(pos_gt)
    pos_pred = np.sum(conf_matrix[:-1, :-1], axis=1).astype(np.float64)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    iou_valid = (pos_gt + pos_pred) > 0
    union = pos_gt + pos_pred - tp
    iou[acc_valid] = tp[acc_valid] / union[acc_valid]
    macc = np.sum(acc[acc_valid]) / np.sum(acc_valid)
    miou = np.sum(iou[acc_valid]) / np.sum(iou_valid)
    fiou = np.sum(iou[acc_valid] * class_weights[acc_valid])
    pacc = np.sum(tp) / np.sum(pos_gt)
    res = {"mIoU": 100 * miou, "fwIoU": 100 * fiou}
    for k, name in enumerate(names):
        res[f"IoU-{name}"] = 100 * iou[k]
    res["mACC"] = 100 * macc
    res["pACC"] = 100 * pacc
    for k, name in enumerate(names):
        res[f"ACC-{name}"] = 100 * acc[k]
    return res


class SemSegEvaluator:
    """``reset()``, ``process(inputs, outputs)`` per batch of images and ``evaluate()``.

    ``process`` pairs the ground truth ``inputs[i]["sem_seg"]`` (an integer array or tensor of labels; or the image
    file ``inputs[i]["sem_seg_file_name"]``, read with PIL) with the prediction ``outputs[i]["sem_seg_labels"]`` (the
    int16 map of ``MaskFormerInference(..., semantic_labels=True)``) or ``outputs[i]["sem_seg"].argmax(0)``, taken on
    the tensor's own device.  A batch is one launch: without ``with_pq`` all images add into one table, with it every
    image has its own and they are summed on the host.  The counting runs on the device of the predictions (or
    ``device``, to which host maps are then uploaded); with everything on the host the numpy definition runs.

    A ground-truth label outside ``[0, num_classes)`` that is not ``ignore_label``, or a predicted label outside
    ``[0, num_classes)``, raises ValueError naming the image (the table's last prediction column exists only to keep
    it square and must stay empty).

    With ``output_dir`` or ``keep_predictions`` ``process`` also collects detectron2's ``sem_seg_predictions.json``
    entries (:func:`bm2f_amd.evaluation.sem_seg_to_coco_json`, one more call per batch; ``file_name`` is the input's
    ``file_name``, else its ``sem_seg_file_name`` or ``image_id``; ``contiguous_id_to_dataset_id`` maps the category
    ids); ``evaluate`` writes them to ``output_dir/sem_seg_predictions.json`` and they stay in ``predictions``.  With
    both left at their defaults nothing is collected and no extra launch runs."""

    def __init__(self, num_classes, ignore_label, class_names=None, device=None, with_pq=False, output_dir=None,
                 keep_predictions=False, contiguous_id_to_dataset_id=None):
        self.output_dir = output_dir
        self.keep_predictions = bool(keep_predictions)
        self.contiguous_id_to_dataset_id = contiguous_id_to_dataset_id
        self.num_classes = int(num_classes)
        self.ignore_label = int(ignore_label)
        if self.num_classes < 1:
            raise ValueError("num_classes must be positive")
        self.class_names = list(class_names) if class_names is not None else [str(k) for k in range(self.num_classes)]
        if len(self.class_names) != self.num_classes:
            raise ValueError(f"{len(self.class_names)} class names for {self.num_classes} classes")
        self.device = torch.device(device) if device is not None else None
        self.with_pq = bool(with_pq)
        self.categories = {k: {"id": k, "name": self.class_names[k], "isthing": 0} for k in range(self.num_classes)}
        self.reset()

    def reset(self):
        n = self.num_classes + 1
        self._counts = np.zeros((n, n), dtype=np.int64)               # [gt row, pred column], as the kernel counts
        self.pq_stat = PQStat(sorted(self.categories)) if self.with_pq else None
        self.num_images = 0
        self.predictions = []                                         # the entries of sem_seg_predictions.json

    @property
    def conf_matrix(self):
        """(K + 1, K + 1) int64 in detectron2's orientation ``[pred, gt]``; index K is the ignore label (as ground
        truth) and stays empty as a prediction."""
        return self._counts.T.copy()

    def _ground_truth(self, inp):
        if "sem_seg" in inp:
            return as_label_plane(inp["sem_seg"], "sem_seg")
        if "sem_seg_file_name" in inp:
            from PIL import Image                                     # only this route needs PIL
            with Image.open(inp["sem_seg_file_name"]) as im:
                return as_label_plane(np.asarray(im), "sem_seg_file_name")
        raise KeyError("an input needs 'sem_seg' or 'sem_seg_file_name'")

    def _prediction(self, out):
        if "sem_seg_labels" in out:
            pred = out["sem_seg_labels"]
        elif "sem_seg" in out:
            scores = out["sem_seg"]
            pred = scores.argmax(0) if torch.is_tensor(scores) else np.asarray(scores).argmax(0)
        else:
            raise KeyError("an output needs 'sem_seg_labels' or 'sem_seg'")
        return as_label_plane(pred, "the prediction", wide=True)

    def _name(self, inp, k):
        for key in ("file_name", "sem_seg_file_name", "image_id"):
            if key in inp:
                return f"{key} {inp[key]!r}"
        return f"number {self.num_images + k} (from reset)"

    def process(self, inputs, outputs):
        inputs, outputs = list(inputs), list(outputs)
        if len(inputs) != len(outputs):
            raise ValueError(f"{len(inputs)} inputs and {len(outputs)} outputs")
        if not inputs:
            return
        gts, preds = [], []
        for k, (inp, out) in enumerate(zip(inputs, outputs)):
            gt, pred = self._ground_truth(inp), self._prediction(out)
            if tuple(gt.shape) != tuple(pred.shape):
                raise ValueError(f"image {self._name(inp, k)}: the prediction is {tuple(pred.shape)}, the ground truth "
                                 f"{tuple(gt.shape)}")
            if self.device is not None:
                pred = (pred if torch.is_tensor(pred) else torch.from_numpy(np.ascontiguousarray(pred))).to(self.device)
            gts.append(gt)
            preds.append(pred)
        n = self.num_classes + 1
        tables, bad = label_pair_counts_ragged(same_dtype(gts), same_dtype(preds), rows=n, cols=n,
                                               ignore=self.ignore_label, share_output=not self.with_pq)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"image {self._name(inputs[k], k)}: {int(bad[k])} pixels hold a ground-truth label outside "
                             f"[0, {self.num_classes}) that is not the ignore label {self.ignore_label}, or a predicted "
                             f"label outside [0, {self.num_classes})")
        last = tables[:, -1] if not self.with_pq else sum(t[:, -1] for t in tables)
        if last.any():
            # the last column exists only to keep the table square: a prediction equal to num_classes is no class.
            # The error path alone reads predictions back, to name the image.
            for k, pred in enumerate(preds):
                flat = pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
                n = int((flat == self.num_classes).sum())
                if n:
                    raise ValueError(f"image {self._name(inputs[k], k)}: {n} pixels hold the predicted label "
                                     f"{self.num_classes}, outside [0, {self.num_classes})")
        if not self.with_pq:
            self._counts += tables
        else:
            for k, table in enumerate(tables):
                self._counts += table
                self.pq_stat += self.image_pq(table, self._name(inputs[k], k))
        if self.output_dir is not None or self.keep_predictions:
            from .evaluation import sem_seg_to_coco_json             # one more call per batch, only when asked for
            self.predictions += sem_seg_to_coco_json(preds, [self._file_name(inp, k) for k, inp in enumerate(inputs)],
                                                     contiguous_id_to_dataset_id=self.contiguous_id_to_dataset_id)
        self.num_images += len(inputs)

    def _file_name(self, inp, k):
        for key in ("file_name", "sem_seg_file_name", "image_id"):
            if key in inp:
                return str(inp[key])
        return str(self.num_images + k)

    def image_pq(self, table, image_id=None):
        """One image's (K + 1, K + 1) table ``[gt, pred]`` -> its PQStat by the rules of the reference tool."""
        present_gt = np.flatnonzero(table[:-1].sum(1)).tolist()
        present_pred = np.flatnonzero(table.sum(0)).tolist()
        gt_segments = [{"id": c, "category_id": c, "iscrowd": 0} for c in present_gt]
        pred_segments = [{"id": c, "category_id": c} for c in present_pred]
        return pq_from_counts(table, gt_segments, pred_segments, self.categories, gt_rows=present_gt,
                              void_row=self.num_classes, void_col=None, image_id=image_id)

    def evaluate(self):
        """-> ``{"sem_seg": {"mIoU", "fwIoU", "mACC", "pACC", "IoU-<name>", "ACC-<name>", ...}}`` x 100 in fp64; with
        ``with_pq`` also ``"PQ"``, ``"SQ"``, ``"RQ"``, ``"PQ-<name>"``, ``"SQ-<name>"``, ``"RQ-<name>"`` x 100 and
        ``"pq_stats"``, the per-class ``tp``, ``fp``, ``fn``, ``iou``."""
        res = sem_seg_metrics(self.conf_matrix, self.class_names)
        if self.output_dir is not None:
            import json
            import os
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, "sem_seg_predictions.json"), "w") as f:
                f.write(json.dumps(self.predictions))
        if self.with_pq:
            avg, per_class = self.pq_stat.pq_average(self.categories)
            for key in ("pq", "sq", "rq"):
                res[key.upper()] = 100 * avg[key]
            for c, r in per_class.items():
                for key in ("pq", "sq", "rq"):
                    res[f"{key.upper()}-{self.class_names[c]}"] = 100 * r[key]
            res["pq_stats"] = self.pq_stat.as_dict()
        return {"sem_seg": res}


def evaluate_sem_seg(ground_truths, predictions, num_classes, ignore_label, class_names=None, device=None,
                     with_pq=False, batch_size=16):
    """Label maps in, metrics out: ``ground_truths`` and ``predictions`` are equally long sequences of integer label
    maps, counted ``batch_size`` images per launch.  -> the ``"sem_seg"`` dict of :meth:`SemSegEvaluator.evaluate`."""
    ev = SemSegEvaluator(num_classes, ignore_label, class_names, device, with_pq)
    ground_truths, predictions = list(ground_truths), list(predictions)
    if len(ground_truths) != len(predictions):
        raise ValueError(f"{len(ground_truths)} ground truths and {len(predictions)} predictions")
    for k in range(0, len(predictions), batch_size):
        ev.process([{"sem_seg": g, "image_id": k + j} for j, g in enumerate(ground_truths[k:k + batch_size])],
                   [{"sem_seg_labels": p} for p in predictions[k:k + batch_size]])
    return ev.evaluate()["sem_seg"]
