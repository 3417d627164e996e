"""bm2f_amd.polygon on the CPU: the vectorised numpy path against the scalar oracle tests/poly_ref.py, the RLE
forms, the refusals and the evaluator's polygons="rasterize".  Every comparison is exact integer or bit equality."""
import copy

import numpy as np
import pytest
import torch

import poly_ref
from bm2f_amd import (COCOEvaluator, COCOGroundTruth, ann_to_rle, convert_polygons_to_rle, evaluate_coco,
                      mask_pair_counts_ragged, polygon_crossings, polygons_to_bits, polygons_to_bits_ragged,
                      polygons_to_rle, rle_decode, rle_encode, rle_to_bits_ragged, unpack_mask_bits)
from bm2f_amd.rle import string_to_counts
from coco_eval_cases import FIELDS, flatten, load_fixture
from polygon_cases import edge_cases, many_parts, pack, polygon_ground_truth

FIXED = [([1, 1, 5, 1, 5, 5, 1, 5], 8, 8, [9, 13, 17, 21, 25, 29, 33, 37, 64], 16),
         ([1, 1, 5, 1, 5, 5], 8, 8, [9, 9, 17, 18, 25, 27, 33, 36, 64], 6),
         ([-2, 3, 6.5, -1, 9, 12, 2.2, 9.7], 8, 7, [2, 7, 9, 16, 17, 24, 25, 32, 32, 40, 40, 48, 48, 56, 56], 50)]


def _planes(words, offsets, sizes):
    words = words.cpu().numpy()
    return [words[o:o + H * ((W + 31) // 32)].reshape(H, -1) for o, (H, W) in zip(offsets, sizes)]


@pytest.mark.parametrize("case", range(3))
def test_fixed_cases(case):
    poly, h, w, positions, area = FIXED[case]
    assert poly_ref.crossings(poly, h, w) == positions                # the oracle itself
    got, off = polygon_crossings([poly], (h, w))
    assert got.dtype == torch.int32 and off.tolist() == [0, len(positions)]
    assert got.tolist() == positions
    mask = unpack_mask_bits(polygons_to_bits([[poly]], (h, w)), w)[0].numpy()
    assert int(mask.sum()) == area and np.array_equal(mask, poly_ref.polygon_mask(poly, h, w))
    if case == 0:
        want = np.zeros((8, 8), dtype=bool)
        want[1:5, 1:5] = True
        assert np.array_equal(mask, want)


def test_sweep_equals_the_oracle():
    cases, ref_pos, ref_mask = poly_ref.sweep_reference()
    assert len(cases) == 2000
    sizes = [(h, w) for _, h, w in cases]
    pos, off = polygon_crossings([p for p, _, _ in cases], sizes)
    assert off[-1] == pos.numel()
    pos = pos.numpy()
    for i in range(len(cases)):
        assert pos[off[i]:off[i + 1]].tolist() == ref_pos[i], i
    words, offsets, hw = polygons_to_bits_ragged([[p] for p, _, _ in cases], sizes)
    assert (offsets % 4 == 0).all() and np.array_equal(hw, np.asarray(sizes))
    for i, plane in enumerate(_planes(words, offsets, hw)):
        assert np.array_equal(plane, pack(ref_mask[i])), i
    assert sum(int(m.any()) for m in ref_mask) > 1500 and sum(int(not m.all()) for m in ref_mask) > 1500


def test_edge_cases_equal_the_oracle():
    cases = edge_cases()
    pos, off = polygon_crossings([p for _, p, _, _ in cases], [(H, W) for _, _, H, W in cases])
    pos = pos.numpy()
    hit_hw = 0
    for i, (name, poly, H, W) in enumerate(cases):
        want = poly_ref.crossings(poly, H, W)
        assert pos[off[i]:off[i + 1]].tolist() == want, name
        hit_hw += name.startswith("clamped_to_h@") and want.count(H * W) >= 2
        if name.startswith("outside"):
            assert want == [H * W], name
        if name.startswith("steep_bisection"):
            assert len(want) > 1, name
    assert hit_hw == 21                                               # a real crossing at p = H * W beside the sentinel


def test_layout_is_that_of_rle_to_bits_ragged():
    anns = [[FIXED[0][0]], [], many_parts(37, 65), [FIXED[2][0], FIXED[1][0]]]
    sizes = [(8, 8), (3, 33), (37, 65), (8, 7)]
    words, offsets, hw = polygons_to_bits_ragged(anns, sizes)
    rles = [rle_encode(torch.from_numpy(poly_ref.annotation_mask(a, h, w))[None])[0] for a, (h, w) in zip(anns, sizes)]
    w2, o2, hw2 = rle_to_bits_ragged(rles)
    assert words.dtype == torch.int32 and torch.equal(words, w2)      # padding words are zero on the CPU
    assert offsets.dtype == np.int64 and np.array_equal(offsets, o2) and np.array_equal(hw, hw2)
    groups = [(h, w, [o], [o]) for o, (h, w) in zip(offsets, sizes)]
    for (inter, area_a, _), a, (h, w) in zip(mask_pair_counts_ragged(words, groups), anns, sizes):
        assert inter[0, 0] == area_a[0] == poly_ref.annotation_mask(a, h, w).sum()
    assert polygons_to_bits_ragged([], [])[0].numel() == 0
    dense = polygons_to_bits([anns[0], anns[1]], (8, 8))
    assert dense.shape == (2, 8, 1) and dense.dtype == torch.int32
    assert np.array_equal(dense[0].numpy(), pack(poly_ref.polygon_mask(FIXED[0][0], 8, 8))) and not dense[1].any()
    assert polygons_to_bits([], (5, 40)).shape == (0, 5, 2)


def test_an_annotation_is_the_union_of_its_parts():
    H, W = 37, 65
    parts = many_parts(H, W, parts=5)
    masks = [poly_ref.polygon_mask(p, H, W) for p in parts]
    union = np.logical_or.reduce(masks)
    xor = np.logical_xor.reduce(masks)
    assert (union != xor).any()                                       # the parts do overlap
    got = unpack_mask_bits(polygons_to_bits([parts, [], parts[:3]], (H, W)), W).numpy()
    assert np.array_equal(got[0], union) and not got[1].any()
    assert np.array_equal(got[2], np.logical_or.reduce(masks[:3]))


def test_rle_forms():
    H, W = 37, 65
    parts = many_parts(H, W, parts=4)
    rles = polygons_to_rle(parts, H, W)
    assert len(rles) == 4 and polygons_to_rle([], H, W) == []
    for r, p in zip(rles, parts):
        mask = poly_ref.polygon_mask(p, H, W)
        assert r == rle_encode(torch.from_numpy(mask)[None])[0]
        assert np.array_equal(rle_decode(r).numpy(), mask)
    united = ann_to_rle(parts, H, W)
    union = poly_ref.annotation_mask(parts, H, W)
    assert united == rle_encode(torch.from_numpy(union)[None])[0]
    assert np.array_equal(rle_decode(united).numpy(), union)
    assert ann_to_rle([], 3, 4) == {"size": [3, 4], "counts": rle_encode(torch.zeros(1, 3, 4, dtype=torch.bool))[0]["counts"]}
    assert ann_to_rle(united, H, W) is united                         # compressed: as it is
    counts = string_to_counts(united["counts"])
    assert ann_to_rle({"size": [H, W], "counts": counts}, H, W) == united
    with pytest.raises(ValueError, match="size"):
        ann_to_rle(united, H, W + 1)
    with pytest.raises(ValueError, match="add up"):
        ann_to_rle({"size": [H, W], "counts": counts[:-1]}, H, W)


def test_refusals():
    ok = [1.0, 1.0, 5.0, 1.0, 5.0, 5.0]
    bad = {"odd": ([ok[:-1] + [2.0, 3.0]], "7 values"), "short": ([ok[:4]], "4 values"),
           "nan": ([ok[:5] + [float("nan")]], "non-finite"), "inf": ([[float("inf")] + ok[1:]], "non-finite"),
           "large": ([ok[:5] + [-2.0 ** 26]], "2\\^26"), "nested": ([[ok]], "flat list"), "dict": ({"counts": 1}, "list")}
    for name, (ann, match) in bad.items():
        with pytest.raises(ValueError, match=match):
            polygons_to_bits([[ok], ann], (8, 8))
        with pytest.raises(ValueError, match="annotation 1: "):       # the annotation is named
            polygons_to_bits_ragged([[ok], ann], [(8, 8), (8, 8)])
    with pytest.raises(ValueError, match="polygon 2"):
        polygon_crossings([ok, ok, ok[:4]], (8, 8))
    with pytest.raises(ValueError, match="polygon 0"):
        polygons_to_rle([ok[:5]], 8, 8)
    assert polygons_to_bits([[ok[:5] + [2.0 ** 26 - 1]]], (8, 8)).shape == (1, 8, 1)
    for size in ((1 << 16, 1 << 15), (0, 5), (5, -1)):
        with pytest.raises(ValueError, match="annotation 0: .*32-bit"):
            polygons_to_bits_ragged([[ok]], [size])
        with pytest.raises(ValueError, match="32-bit"):
            polygons_to_bits([[ok]], size)
    with pytest.raises(ValueError, match="sizes"):
        polygons_to_bits_ragged([[ok], [ok]], [(8, 8)])
    gt = copy.deepcopy(load_fixture()[0])
    gt["annotations"][2]["segmentation"] = [ok[:5]]
    name = f"annotation {gt['annotations'][2]['id']}: "
    with pytest.raises(ValueError, match=name):
        convert_polygons_to_rle(gt)
    with pytest.raises(ValueError, match=name):                       # before any batch is counted
        evaluate_coco(COCOGroundTruth(gt, polygons="rasterize"), load_fixture()[1])
    with pytest.raises(ValueError, match="polygons"):
        COCOGroundTruth(gt, polygons="maybe")


def _flat(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, 10)


def _same(a, b):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f


def test_the_default_still_refuses_polygons():
    poly_gt, _, _ = polygon_ground_truth()
    with pytest.raises(NotImplementedError, match="RLE"):
        COCOGroundTruth(copy.deepcopy(poly_gt))
    with pytest.raises(NotImplementedError, match="RLE"):
        COCOEvaluator(copy.deepcopy(poly_gt))
    assert COCOGroundTruth(load_fixture()[0]).polygons == "refuse"


def test_evaluator_with_polygon_ground_truth_equals_the_oracle_rle():
    poly_gt, rle_gt, results = polygon_ground_truth()
    before = copy.deepcopy(poly_gt)
    want = _flat(evaluate_coco(COCOGroundTruth(rle_gt), results))
    for kw in ({}, {"batch_bytes": 300_000}, {"batch_bytes": 1}):
        _same(_flat(evaluate_coco(COCOGroundTruth(poly_gt, polygons="rasterize"), results, **kw)), want)
    assert poly_gt == before
    assert want["stats"][0] > 0
    ev = COCOEvaluator(poly_gt, polygons="rasterize")
    ev.reset()
    ev._predictions = [dict(r) for r in results]
    ev.evaluate()
    assert np.array_equal(ev.last["segm"].stats, want["stats"])


def test_converting_once_equals_rasterizing_in_the_evaluator():
    poly_gt, rle_gt, results = polygon_ground_truth()
    before = copy.deepcopy(poly_gt)
    converted = convert_polygons_to_rle(poly_gt)
    assert poly_gt == before and converted["annotations"] == rle_gt["annotations"]
    assert convert_polygons_to_rle(poly_gt, batch_bytes=1)["annotations"] == rle_gt["annotations"]
    a = evaluate_coco(COCOGroundTruth(converted), results)            # default settings read the converted file
    b = evaluate_coco(COCOGroundTruth(poly_gt, polygons="rasterize"), results)
    assert np.array_equal(a.stats, b.stats)
    assert a.ious.keys() == b.ious.keys()
    for k in a.ious:
        assert np.array_equal(np.asarray(a.ious[k]), np.asarray(b.ious[k])), k
    _same(_flat(a), _flat(b))
