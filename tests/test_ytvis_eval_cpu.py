"""Video AP on the host (no GPU): evaluate_ytvis against fixtures made by the reference's YTVOS / YTVOSeval
(tests/golden/gen_ytvis_eval_golden.py, which asserts the branches the data reaches), the ground-truth index, and
YTVISEvaluator end to end on the video head's CPU outputs."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from bm2f_amd import (VideoMaskFormerInference, YTVISEvaluator, YTVISGroundTruth, YTVISParams, evaluate_ytvis,
                      instances_to_coco_json_video, rle_encode)
from ytvis_eval_cases import CONFIGS, FIELDS, GT_JSON, flatten, load_fixture

GT, RESULTS, EXPECTED = load_fixture()


def flat_result(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, len(r.params.iouThrs))


def assert_matches_fixture(got, want):
    """ious, every evalImgs field, precision, recall and scores equal exactly; stats within 1e-9: they are fp64 means
    of at most ~1e5 values in [-1, 1], so reordering the sum moves them by less than 1e5 * 2^-53."""
    for f in FIELDS:
        if f == "stats":
            assert np.abs(got[f] - want[f]).max() <= 1e-9, f
        else:
            assert got[f].shape == want[f].shape, f
            assert np.array_equal(got[f], want[f]), f


def params_for(name):
    p = YTVISParams()
    p.maxDets = list(CONFIGS[name])
    return p


@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_ytvis_equals_reference(name):
    r = evaluate_ytvis(YTVISGroundTruth(copy.deepcopy(GT)), copy.deepcopy(RESULTS), params=params_for(name))
    assert_matches_fixture(flat_result(r), EXPECTED[name])
    assert r.precision.shape == (10, 101, 4, 4, 3) and r.recall.shape == (10, 4, 4, 3) and r.stats.shape == (12,)


def test_fixture_reaches_the_summary_edges():
    want = EXPECTED["default"]
    assert (want["precision"][:, :, 3] == -1).all()                   # the category without any instance
    assert want["stats"][0] > 0 and EXPECTED["reduced"]["stats"][0] == -1   # stats[0] asks for maxDets == 100
    assert (want["iou_values"] == 0.5).any()
    assert EXPECTED["reduced"]["img_nd"].max() == 5 and want["img_nd"].max() == 7


def test_ground_truth_from_path_and_inputs_are_not_modified():
    gt_dict, results = copy.deepcopy(GT), copy.deepcopy(RESULTS)
    r = evaluate_ytvis(YTVISGroundTruth(GT_JSON), results)
    assert_matches_fixture(flat_result(r), EXPECTED["default"])
    evaluate_ytvis(YTVISGroundTruth(gt_dict), results)
    assert gt_dict == GT and results == RESULTS


def test_unsupported_settings_raise():
    gt = YTVISGroundTruth(copy.deepcopy(GT))
    p = YTVISParams()
    p.iouType = "bbox"
    with pytest.raises(NotImplementedError):
        evaluate_ytvis(gt, RESULTS, params=p)
    p = YTVISParams()
    p.useCats = 0
    with pytest.raises(NotImplementedError):
        evaluate_ytvis(gt, RESULTS, params=p)
    poly = copy.deepcopy(GT)
    poly["annotations"][0]["segmentations"][0] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    with pytest.raises(NotImplementedError):
        YTVISGroundTruth(poly)
    with pytest.raises(ValueError):
        evaluate_ytvis(gt, [dict(RESULTS[0], video_id=999)])
    bad = copy.deepcopy(RESULTS[:1])
    bad[0]["segmentations"] = bad[0]["segmentations"][:1]             # one frame for a two-frame video
    with pytest.raises(ValueError):
        evaluate_ytvis(gt, bad)


def _video_outputs(Q=12, K=3, T=2, h=20, w=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, Q, T, 3, 4, generator=g) * 3                 # blobs: connected regions after upsampling
    masks = torch.nn.functional.interpolate(low.flatten(0, 1), size=(h, w), mode="bilinear").view(1, Q, T, h, w)
    return {"pred_logits": torch.randn(1, Q, K + 1, generator=g) * 2, "pred_masks": masks}


def _head_dataset():
    """Two videos run through the head; the ground truth is made of some of the head's own masks (so they match
    exactly), one of them shifted, in dataset category ids 11, 12, 13 for the contiguous 0, 1, 2."""
    head = VideoMaskFormerInference(3, test_topk_per_video=6)
    id_map = {11: 0, 12: 1, 13: 2}
    geometry = ((80, 112), (75, 100))
    videos, anns, outs = [], [], []
    for vid, seed in ((5, 0), (9, 1)):
        out = _video_outputs(seed=seed)
        plain = head(out, *geometry)
        videos.append({"id": vid, "height": 75, "width": 100, "length": 2})
        order = np.argsort(plain["pred_scores"])[::-1]
        for rank, e in enumerate(order[:3]):
            m = plain["pred_masks"][e]
            if rank == 1:
                m = torch.roll(m, shifts=9, dims=-1)
            anns.append({"id": len(anns) + 1, "video_id": vid, "category_id": plain["pred_labels"][e] + 11,
                         "iscrowd": 0, "segmentations": rle_encode(m), "areas": [int(f.sum()) for f in m]})
        outs.append((vid, out))
    gt = {"videos": videos, "annotations": anns,
          "categories": [{"id": 11, "name": "a"}, {"id": 12, "name": "b"}, {"id": 13, "name": "c"}]}
    return head, geometry, id_map, gt, outs


def _same(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)


def test_evaluator_end_to_end_in_every_output_form():
    head, geometry, id_map, gt, outs = _head_dataset()
    metrics, results = [], []
    for kw in ({}, {"packed": True}, {"rle": True}, {"keep_bits": True}, {"rle": True, "keep_bits": True}):
        ev = YTVISEvaluator(copy.deepcopy(gt), thing_dataset_id_to_contiguous_id=id_map, class_names=["a", "b", "c"])
        ev.reset()
        for vid, out in outs:
            ev.process([{"video_id": vid, "length": 2}], head(out, *geometry, **kw))
        m = ev.evaluate()
        assert set(m) == {"segm"}
        assert set(m["segm"]) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AP-a", "AP-b", "AP-c"}
        metrics.append(m["segm"])
        results.append(ev.results)
        assert json.loads(json.dumps(ev.results)) == ev.results and len(ev.results) == 12
        assert all(0 <= r["category_id"] <= 2 for r in ev.results)    # results.json keeps the head's ids
    for m in metrics[1:]:
        assert _same(m, metrics[0])
    assert all(r == results[0] for r in results[1:])
    assert metrics[0]["AP50"] > 0 and metrics[0]["AP"] <= metrics[0]["AP50"] <= 100
    assert math.isnan(metrics[0]["APl"])                              # nothing of 256^2 pixels in a 75 x 100 frame
    # the same numbers from evaluate_ytvis on the written results, mapped to dataset ids
    mapped = [dict(r, category_id=r["category_id"] + 11) for r in results[0]]
    direct = evaluate_ytvis(YTVISGroundTruth(gt), mapped)
    assert direct.stats[1] * 100 == metrics[0]["AP50"]


def test_evaluator_without_predictions_or_annotations():
    _, _, id_map, gt, _ = _head_dataset()
    assert YTVISEvaluator(gt, id_map).evaluate() == {}
    no_ann = {k: v for k, v in gt.items() if k != "annotations"}
    ev = YTVISEvaluator(no_ann, id_map)
    head = VideoMaskFormerInference(3, test_topk_per_video=6)
    ev.process([{"video_id": 5, "length": 2}], head(_video_outputs(), (80, 112), (75, 100), keep_bits=True))
    assert ev.evaluate() == {} and len(ev.results) == 6


def test_keep_bits_on_cpu_is_the_packed_output():
    head = VideoMaskFormerInference(3, test_topk_per_video=6)
    out = _video_outputs()
    args = (out, (80, 112), (75, 100), (90, 130))
    packed = head(*args, packed=True)
    for kw in ({}, {"packed": True}, {"rle": True}):
        r = head(*args, keep_bits=True, **kw)
        assert torch.equal(r["pred_bits"], torch.stack(packed["pred_masks"]))
        assert r["pred_bits"].dtype == torch.int32 and tuple(r["pred_bits"].shape) == (6, 2, 90, 5)
        plain = head(*args, **kw)
        assert "pred_bits" not in plain
        assert instances_to_coco_json_video([{"video_id": 1}], plain) == \
            instances_to_coco_json_video([{"video_id": 1}], r)
