"""Image AP on the host (no GPU): evaluate_coco against fixtures whose matching, accumulation and summary are the
reference's YTVOSeval run on one-frame videos with dense COCO IoUs (tests/golden/gen_coco_eval_golden.py, which
asserts the branches the data reaches), COCOEvaluator end to end, the refusals, and the ragged decoder on the CPU."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from bm2f_amd import (COCOEvalResult, COCOEvaluator, COCOGroundTruth, COCOParams, evaluate_coco,
                      mask_pair_counts_ragged, pack_mask_bits, rle_encode, rle_to_bits, rle_to_bits_ragged,
                      string_to_counts)
from coco_eval_cases import CONFIGS, FIELDS, GT_JSON, flatten, load_fixture

GT, RESULTS, EXPECTED = load_fixture()


def flat_result(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, len(r.params.iouThrs))


def assert_matches_fixture(got, want):
    """Every field, stats included, equals the fixture exactly: the IoUs are ratios of the same integers and the
    summary runs the same numpy operations in the same order as the oracle."""
    for f in FIELDS:
        assert got[f].shape == want[f].shape, f
        assert np.array_equal(got[f], want[f]), f


def run(name, **kw):
    max_dets, iou_type = CONFIGS[name]
    p = COCOParams(iou_type)
    p.maxDets = list(max_dets)
    return evaluate_coco(COCOGroundTruth(copy.deepcopy(GT)), copy.deepcopy(RESULTS), iou_type=iou_type, params=p, **kw)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_coco_equals_oracle(name):
    r = run(name)
    assert isinstance(r, COCOEvalResult)
    assert_matches_fixture(flat_result(r), EXPECTED[name])
    assert r.precision.shape == (10, 101, 4, 4, 3) and r.recall.shape == (10, 4, 4, 3) and r.stats.shape == (12,)
    assert all("image_id" in e and "video_id" not in e for e in r.evalImgs if e is not None)


def test_batch_size_does_not_change_the_result():
    whole = flat_result(run("default"))
    for batch_bytes in (1, 100_000, 1 << 20):
        got = flat_result(run("default", batch_bytes=batch_bytes))
        assert all(np.array_equal(got[f], whole[f]) for f in FIELDS)


def test_fixture_reaches_the_summary_edges():
    want = EXPECTED["default"]
    assert (want["precision"][:, :, 3] == -1).all()                   # the category without any instance
    assert want["stats"][0] > 0 and EXPECTED["reduced"]["stats"][0] == -1   # stats[0] asks for maxDets == 100
    assert (want["iou_values"] == 0.5).any() and (want["iou_values"] == 1.0).any()   # 1.0: the crowd rule
    assert EXPECTED["reduced"]["img_nd"].max() == 5 and want["img_nd"].max() == 7
    assert all((want["stats"][3:6] > -1)) and all(want["stats"][9:12] > -1)   # small, medium and large occur


def test_ground_truth_from_path_and_inputs_are_not_modified():
    gt_dict, results = copy.deepcopy(GT), copy.deepcopy(RESULTS)
    r = evaluate_coco(COCOGroundTruth(GT_JSON), results)
    assert_matches_fixture(flat_result(r), EXPECTED["default"])
    evaluate_coco(COCOGroundTruth(gt_dict), results, iou_type="bbox")
    assert gt_dict == GT and results == RESULTS


def test_area_comes_from_the_annotation_field():
    """Doubling every area field moves ground truths between ranges; the mask IoUs do not change."""
    gt = copy.deepcopy(GT)
    for a in gt["annotations"]:
        a["area"] *= 4
    base = run("default")
    r = evaluate_coco(COCOGroundTruth(gt), copy.deepcopy(RESULTS))
    assert all(np.array_equal(r.ious[k], base.ious[k]) for k in base.ious)
    assert not np.array_equal(r.stats[3:6], base.stats[3:6])


def test_refusals():
    gt = COCOGroundTruth(copy.deepcopy(GT))
    poly = copy.deepcopy(GT)
    poly["annotations"][2]["segmentation"] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    with pytest.raises(NotImplementedError, match=f"annotation {poly['annotations'][2]['id']} .*RLE"):
        COCOGroundTruth(poly)
    with pytest.raises(ValueError, match="images"):
        evaluate_coco(gt, [dict(RESULTS[0], image_id=999)])
    bad = copy.deepcopy(RESULTS[:1])
    other = next(im for im in GT["images"] if [im["height"], im["width"]] != bad[0]["segmentation"]["size"])
    bad[0]["image_id"] = other["id"]
    with pytest.raises(ValueError, match="size"):
        evaluate_coco(gt, bad)
    nobox = copy.deepcopy(RESULTS)
    del nobox[3]["bbox"]
    with pytest.raises(ValueError, match="bbox"):
        evaluate_coco(gt, nobox, iou_type="bbox")
    evaluate_coco(gt, nobox)                                          # masks do not need it
    p = COCOParams()
    p.useCats = 0
    with pytest.raises(NotImplementedError):
        evaluate_coco(gt, RESULTS, params=p)
    with pytest.raises(NotImplementedError):
        evaluate_coco(gt, RESULTS, iou_type="keypoints")


def test_empty_result_list():
    gt = COCOGroundTruth(copy.deepcopy(GT))
    r = evaluate_coco(gt, [])
    assert r.stats[0] == 0 and r.stats[8] == 0                        # ground truth and nothing found
    assert (r.precision[:, :, 3] == -1).all()
    ev = COCOEvaluator(gt, class_names=["person", "dog", "car", "kite"], tasks=("bbox", "segm"))
    m = ev.evaluate()
    assert set(m) == {"bbox", "segm"} and ev.last == {"bbox": None, "segm": None}
    assert all(math.isnan(v) for task in m.values() for v in task.values())
    no_ann = {k: v for k, v in GT.items() if k != "annotations"}
    assert COCOEvaluator(no_ann).evaluate() == {}


def test_evaluator_end_to_end_with_a_category_mapping():
    """Instances as the image head returns them (contiguous class ids, XYXY boxes, RLE or bool masks), dataset ids
    11.. in the ground truth."""
    id_map = {c["id"] + 10: c["id"] - 1 for c in GT["categories"]}
    gt = copy.deepcopy(GT)
    for a in gt["annotations"]:
        a["category_id"] += 10
    for c in gt["categories"]:
        c["id"] += 10
    names = [c["name"] for c in GT["categories"]]
    by_image = {}
    for r in RESULTS:
        by_image.setdefault(r["image_id"], []).append(r)
    metrics = []
    for as_rle in (True, False):
        ev = COCOEvaluator(gt, thing_dataset_id_to_contiguous_id=id_map, class_names=names, tasks=("segm", "bbox"))
        ev.reset()
        for img_id, rs in by_image.items():
            boxes = torch.tensor([r["bbox"] for r in rs])
            boxes[:, 2:] += boxes[:, :2]
            inst = {"scores": torch.tensor([r["score"] for r in rs], dtype=torch.float64),
                    "pred_classes": torch.tensor([r["category_id"] - 1 for r in rs]), "pred_boxes": boxes}
            if as_rle:
                inst["pred_masks_rle"] = [r["segmentation"] for r in rs]
            else:
                planes = torch.stack([rle_to_bits([r["segmentation"]])[0] for r in rs])
                W = rs[0]["segmentation"]["size"][1]
                bits = (planes[..., None] >> torch.arange(32)) & 1
                inst["pred_masks"] = bits.flatten(-2)[..., :W].bool()
            ev.process([{"image_id": img_id}], [{"instances": inst}])
        m = ev.evaluate()
        assert set(m) == {"segm", "bbox"}
        assert set(m["segm"]) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10"} | {"AP-" + n for n in names}
        assert json.loads(json.dumps(ev.results)) == ev.results and len(ev.results) == len(RESULTS)
        assert all(0 <= r["category_id"] <= 3 for r in ev.results)    # the results keep the head's ids
        metrics.append(m)
    assert metrics[0] == metrics[1] or all(
        a == b or (math.isnan(a) and math.isnan(b))
        for t in metrics[0] for a, b in zip(metrics[0][t].values(), metrics[1][t].values()))
    m = metrics[0]
    assert m["segm"]["AP"] == EXPECTED["default"]["stats"][0] * 100 and math.isnan(m["segm"]["AP-kite"])
    assert m["bbox"]["AP50"] == EXPECTED["bbox"]["stats"][1] * 100
    # a class outside the mapping is refused as the reference does
    ev = COCOEvaluator(gt, thing_dataset_id_to_contiguous_id=id_map)
    ev.process([{"image_id": 1}], [{"instances": {"scores": [0.5], "pred_classes": [7],
                                                   "pred_boxes": torch.zeros(1, 4),
                                                   "pred_masks_rle": [RESULTS[0]["segmentation"]]}}])
    with pytest.raises(AssertionError, match="class=7"):
        ev.evaluate()


RAGGED_SIZES = [(1, 1), (2, 31), (7, 32), (3, 33), (5, 64), (4, 65), (70, 2100), (9, 127)]


def ragged_masks():
    g = torch.Generator().manual_seed(3)
    masks = [torch.rand(h, w, generator=g) < p for (h, w), p in zip(RAGGED_SIZES, (0.5, 0.5, 0.1, 0.9, 0.5, 0.5, 0.3, 0.5))]
    masks[2] = torch.zeros(7, 32, dtype=torch.bool)
    masks[3] = torch.ones(3, 33, dtype=torch.bool)
    return masks


def test_rle_to_bits_ragged_on_cpu():
    masks = ragged_masks()
    rles = [rle_encode(m[None])[0] for m in masks]
    rles[4] = dict(rles[4], counts=string_to_counts(rles[4]["counts"]))     # uncompressed
    rles.append(None)
    sizes = [None] * len(masks) + [(6, 40)]
    words, offsets, hw = rle_to_bits_ragged(rles, sizes=sizes)
    assert words.dtype == torch.int32 and words.dim() == 1 and (offsets % 4 == 0).all()
    assert hw.tolist() == [list(s) for s in RAGGED_SIZES] + [[6, 40]]
    covered = torch.zeros(words.numel(), dtype=torch.bool)
    for m, r in enumerate(rles):
        H, W = hw[m]
        alone = rle_to_bits([r], size=(H, W))
        n = alone.numel()
        assert torch.equal(words[offsets[m]:offsets[m] + n].view(alone.shape), alone)
        if r is not None:
            assert torch.equal(alone[0], pack_mask_bits(masks[m][None])[0])
        assert not covered[offsets[m]:offsets[m] + n].any()
        covered[offsets[m]:offsets[m] + n] = True
    assert int(words[~covered].abs().sum()) == 0
    with pytest.raises(ValueError):
        rle_to_bits_ragged(rles)                                      # the None entry has no size
    with pytest.raises(ValueError):
        rle_to_bits_ragged(rles[:2], sizes=[(1, 1), (3, 31)])         # contradicts the mask's own size
    with pytest.raises(ValueError):
        rle_to_bits_ragged([{"size": [7, 33], "counts": [5, 5]}])
    assert rle_to_bits_ragged([])[0].numel() == 0


def test_mask_pair_counts_ragged_on_cpu():
    masks = ragged_masks()
    words, offsets, _ = rle_to_bits_ragged([rle_encode(m[None])[0] for m in masks])
    big, odd = offsets[6], offsets[7]
    got = mask_pair_counts_ragged(words, [(70, 2100, [big, big], [big]), (9, 127, [odd], []), (1, 1, [], [])])
    area = int(masks[6].sum())
    assert np.array_equal(got[0][0], [[area], [area]]) and np.array_equal(got[0][1], [area, area])
    assert got[1][0].shape == (1, 0) and got[1][1].tolist() == [int(masks[7].sum())] and got[1][2].shape == (0,)
    assert got[2][0].shape == (0, 0)
    assert all(a.dtype == np.int64 for g in got for a in g)
    for bad in ([(70, 2100, [words.numel() - 10], [])], [(0, 5, [], [])], [(3, 3, [-1], [])], [(3, 3, [0])]):
        with pytest.raises(ValueError):
            mask_pair_counts_ragged(words, bad)
    with pytest.raises(ValueError):
        mask_pair_counts_ragged(words.long(), [(1, 1, [0], [0])])


def test_rle_pair_counts_ragged_equals_the_two_steps():
    """The evaluator's batch step (one upload for both kernels) against rle_to_bits_ragged + mask_pair_counts_ragged,
    with a None entry sized by ``sizes``."""
    from bm2f_amd.mask_iou import rle_pair_counts_ragged
    masks = ragged_masks()
    rles = [rle_encode(m[None])[0] for m in masks] + [None]
    sizes = [None] * len(masks) + [(9, 127)]
    by_index = [(70, 2100, [6, 6], [6]), (9, 127, [7, 8], [8, 7]), (3, 33, [], [3]), (1, 1, [], [])]
    words, off, _ = rle_to_bits_ragged(rles, sizes=sizes)
    want = mask_pair_counts_ragged(words, [(H, W, off[ia], off[ib]) for H, W, ia, ib in by_index])
    got = rle_pair_counts_ragged(rles, by_index, sizes=sizes)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(np.array_equal(x, y) and x.dtype == np.int64 for x, y in zip(g, w))
    assert got[1][0][0, 0] == 0 and got[1][0][0, 1] == int(masks[7].sum())      # the None plane is empty
    with pytest.raises(ValueError):
        rle_pair_counts_ragged(rles, [(9, 127, [6], [])], sizes=sizes)          # a mask of another size
    with pytest.raises(ValueError):
        rle_pair_counts_ragged(rles, [(9, 127, [99], [])], sizes=sizes)
    assert rle_pair_counts_ragged(rles, [], sizes=sizes) == []


def test_word_limit_is_a_value_error_before_anything_is_allocated():
    """2^31 - 1 words per buffer: refused on the host, and image_batches never builds such a batch."""
    from bm2f_amd.coco_eval import image_batches
    from bm2f_amd.mask_iou import MAX_RAGGED_WORDS, rle_pair_counts_ragged
    side = 40000                                                      # 1.6e9 pixels, 5e7 words per plane
    big = [{"size": [side, side], "counts": [side * side]} for _ in range(50)]
    assert 50 * side * (side // 32) > MAX_RAGGED_WORDS
    with pytest.raises(ValueError, match="words"):
        rle_to_bits_ragged(big)
    with pytest.raises(ValueError, match="words"):
        rle_pair_counts_ragged(big, [(side, side, list(range(50)), [])])
    gt = COCOGroundTruth({"images": [{"id": i, "height": side, "width": side} for i in range(3)], "categories": [],
                          "annotations": [{"id": i * 20 + k, "image_id": i, "category_id": 1, "segmentation": big[0]}
                                          for i in range(3) for k in range(20)]})
    assert image_batches(gt, [0, 1, 2], {}, 1 << 60) == [[0, 1], [2]]   # 2e8 bytes per plane, 20 planes per image


def test_chunked_parse_equals_the_whole_parse(monkeypatch):
    """_decode_plan parses long batches in runs of masks; any cut gives the same run ends and offsets."""
    import importlib
    mi = importlib.import_module("bm2f_amd.mask_iou")
    masks = ragged_masks()
    rles = [rle_encode(m[None])[0] for m in masks]
    rles[1] = dict(rles[1], counts=string_to_counts(rles[1]["counts"]))
    rles = rles[:3] + [None] + rles[3:] + [None]
    sizes = [None] * 3 + [(2, 2)] + [None] * 5 + [(1, 40)]
    hw = mi._ragged_sizes(rles, sizes)
    pos, off = mi._run_ends_sized(rles, hw[:, 0] * hw[:, 1])
    for chunk in (1, 7, 40, 3000):
        monkeypatch.setattr(mi, "_PARSE_CHUNK", chunk)
        p, o = mi._run_ends_chunked(rles, hw[:, 0] * hw[:, 1])
        assert p.dtype == pos.dtype and o.dtype == off.dtype
        assert np.array_equal(p, pos) and np.array_equal(o, off), chunk
        words, _, _ = rle_to_bits_ragged(rles, sizes=sizes)
        monkeypatch.setattr(mi, "_PARSE_CHUNK", 1 << 20)
        assert torch.equal(words, rle_to_bits_ragged(rles, sizes=sizes)[0])
