"""The kernels of csrc/polygon.hip on the device against the scalar oracle tests/poly_ref.py, and the evaluator's
polygons="rasterize" on the device against its CPU run.  Every comparison is exact integer or bit equality."""
import copy

import numpy as np
import pytest
import torch

import poly_ref
from bm2f_amd import (COCOGroundTruth, _native, ann_to_rle, convert_polygons_to_rle, evaluate_coco, mask_pair_counts,
                      mask_pair_counts_ragged, polygon_crossings, polygons_to_bits, polygons_to_bits_ragged,
                      polygons_to_rle, rle_encode)
from coco_eval_cases import FIELDS, flatten, load_fixture
from polygon_cases import edge_cases, many_parts, pack, polygon_ground_truth

pytestmark = pytest.mark.gpu


def _planes(words, offsets, sizes):
    words = words.cpu().numpy()
    return [words[o:o + H * ((W + 31) // 32)].reshape(H, -1) for o, (H, W) in zip(offsets, sizes)]


def test_sweep_equals_the_oracle(device):
    cases, ref_pos, ref_mask = poly_ref.sweep_reference()
    sizes = [(h, w) for _, h, w in cases]
    pos, off = polygon_crossings([p for p, _, _ in cases], sizes, device=device)
    assert pos.device.type == "cuda" and pos.dtype == torch.int32 and off[-1] == pos.numel()
    pos = pos.cpu().numpy()
    for i in range(len(cases)):
        assert pos[off[i]:off[i + 1]].tolist() == ref_pos[i], i
    words, offsets, hw = polygons_to_bits_ragged([[p] for p, _, _ in cases], sizes, device=device)
    assert words.device.type == "cuda" and words.dtype == torch.int32 and (offsets % 4 == 0).all()
    for i, plane in enumerate(_planes(words, offsets, hw)):
        assert np.array_equal(plane, pack(ref_mask[i])), i             # word for word: the tail bits are zero


def test_edge_cases_equal_the_oracle(device):
    """W in {1, 31, 32, 33, 64, 65, 257} x H in {1, 2, 37}: polygons outside the image, rows clamped to H in a middle
    and in the last column (p = H W), zero-length and vertical edges, a steep edge of 5 H steps and one fifth of a
    column (the bisection), integer and half-integer ties."""
    cases = edge_cases()
    sizes = [(H, W) for _, _, H, W in cases]
    pos, off = polygon_crossings([p for _, p, _, _ in cases], sizes, device=device)
    pos = pos.cpu().numpy()
    for i, (name, poly, H, W) in enumerate(cases):
        assert pos[off[i]:off[i + 1]].tolist() == poly_ref.crossings(poly, H, W), name
    words, offsets, hw = polygons_to_bits_ragged([[p] for _, p, _, _ in cases], sizes, device=device)
    for (name, poly, H, W), plane in zip(cases, _planes(words, offsets, hw)):
        assert np.array_equal(plane, pack(poly_ref.polygon_mask(poly, H, W))), name


def test_many_parts_and_no_parts_among_images_of_different_sizes(device):
    sizes = [(37, 65), (3, 33), (70, 300), (8, 7), (37, 65), (130, 257)]
    anns = [many_parts(37, 65, 20), [], many_parts(70, 300, 20, seed=6), [[-2, 3, 6.5, -1, 9, 12, 2.2, 9.7]], [],
            many_parts(130, 257, 7, seed=7)]
    words, offsets, hw = polygons_to_bits_ragged(anns, sizes, device=device)
    cpu = polygons_to_bits_ragged(anns, sizes)
    assert np.array_equal(offsets, cpu[1]) and np.array_equal(hw, cpu[2]) and words.numel() == cpu[0].numel()
    want = [poly_ref.annotation_mask(a, H, W) for a, (H, W) in zip(anns, sizes)]
    union_differs = False
    for m, (plane, c) in enumerate(zip(_planes(words, offsets, hw), _planes(cpu[0], offsets, hw))):
        assert np.array_equal(plane, pack(want[m])) and np.array_equal(plane, c), m
        if len(anns[m]) > 1:
            xor = np.logical_xor.reduce([poly_ref.polygon_mask(p, *sizes[m]) for p in anns[m]])
            union_differs |= bool((xor != want[m]).any())
    assert union_differs and not want[1].any() and want[0].any()
    # the padding words between planes are ignored by the pair counts, whatever they hold
    groups = [(H, W, [o], [o]) for o, (H, W) in zip(offsets, sizes)]
    for (inter, area_a, area_b), w in zip(mask_pair_counts_ragged(words, groups), want):
        assert inter[0, 0] == area_a[0] == area_b[0] == w.sum()
    # one annotation alone and inside the batch give the same plane
    alone = polygons_to_bits_ragged([anns[2]], [sizes[2]], device=device)[0].cpu().numpy()
    assert np.array_equal(alone[:70 * 10].reshape(70, 10), pack(want[2]))


def test_polygons_to_bits_feeds_mask_pair_counts(device):
    H, W = 37, 65
    a = [many_parts(H, W, 3, seed=s) for s in range(5)]
    b = [many_parts(H, W, 2, seed=10 + s) for s in range(3)] + [[]]
    pa, pb = polygons_to_bits(a, (H, W), device=device), polygons_to_bits(b, (H, W), device=device)
    assert pa.shape == (5, H, 3) and pa.dtype == torch.int32 and pa.device.type == "cuda"
    ma = np.stack([poly_ref.annotation_mask(x, H, W) for x in a])
    mb = np.stack([poly_ref.annotation_mask(x, H, W) for x in b])
    inter, area_a, area_b = mask_pair_counts(pa[:, None], pb[:, None], W)
    assert np.array_equal(inter, (ma[:, None] & mb[None]).sum((2, 3)))
    assert np.array_equal(area_a.reshape(-1), ma.sum((1, 2))) and np.array_equal(area_b.reshape(-1), mb.sum((1, 2)))
    assert torch.equal(pa.cpu(), polygons_to_bits(a, (H, W)))


def test_rle_forms_on_the_device(device):
    H, W = 70, 300
    parts = many_parts(H, W, 4, seed=6)
    want = [rle_encode(torch.from_numpy(poly_ref.polygon_mask(p, H, W))[None])[0] for p in parts]
    assert polygons_to_rle(parts, H, W, device=device) == want
    union = rle_encode(torch.from_numpy(poly_ref.annotation_mask(parts, H, W))[None])[0]
    assert ann_to_rle(parts, H, W, device=device) == union
    poly_gt, rle_gt, _ = polygon_ground_truth()
    assert convert_polygons_to_rle(poly_gt, device=device)["annotations"] == rle_gt["annotations"]


def _flat(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, 10)


def test_evaluator_on_a_mixed_batch_equals_the_cpu_run(device):
    poly_gt, rle_gt, results = polygon_ground_truth()
    cpu = _flat(evaluate_coco(COCOGroundTruth(copy.deepcopy(poly_gt), polygons="rasterize"), results))
    oracle = _flat(evaluate_coco(COCOGroundTruth(rle_gt), results))
    for kw in ({}, {"batch_bytes": 300_000}, {"batch_bytes": 1}):
        gt = COCOGroundTruth(copy.deepcopy(poly_gt), polygons="rasterize")
        got = _flat(evaluate_coco(gt, results, device=device, **kw))
        for f in FIELDS:
            assert np.array_equal(got[f], cpu[f]), (f, kw)
            assert np.array_equal(got[f], oracle[f]), (f, kw)


class _Counter:
    """Records the native calls, the uploads, the sorts and the device-to-host copies of a block of code."""

    def __init__(self, monkeypatch):
        self.calls, self.uploads, self.sorts, self.copies = [], 0, 0, 0
        real_call, real_upload, real_sort, real_cpu = _native.call, _native.upload_tables, torch.sort, torch.Tensor.cpu

        def call(name, *args):
            self.calls.append(name)
            return real_call(name, *args)

        def upload(tables, device):
            self.uploads += 1
            return real_upload(tables, device)

        def sort(*args, **kw):
            self.sorts += 1
            return real_sort(*args, **kw)

        def cpu(t, *args, **kw):
            self.copies += t.device.type == "cuda"
            return real_cpu(t, *args, **kw)

        monkeypatch.setattr(_native, "call", call)
        monkeypatch.setattr(_native, "upload_tables", upload)
        monkeypatch.setattr(torch, "sort", sort)
        monkeypatch.setattr(torch.Tensor, "cpu", cpu)


def _subset(gt, results, image_ids):
    gt = copy.deepcopy(gt)
    gt["images"] = [im for im in gt["images"] if im["id"] in image_ids]
    gt["annotations"] = [a for a in gt["annotations"] if a["image_id"] in image_ids]
    return gt, [r for r in results if r["image_id"] in image_ids]


def test_launches_and_copies_do_not_grow_with_the_batch(device, monkeypatch):
    poly_gt, _, results = polygon_ground_truth()
    with_polys = [im["id"] for im in poly_gt["images"]
                  if any(a["image_id"] == im["id"] and isinstance(a["segmentation"], list)
                         for a in poly_gt["annotations"])]
    assert len(with_polys) >= 6
    seen = []
    for n in (2, 6):
        gt, res = _subset(poly_gt, results, set(with_polys[:n]))
        ground_truth = COCOGroundTruth(gt, polygons="rasterize")
        with monkeypatch.context() as mp:
            c = _Counter(mp)
            evaluate_coco(ground_truth, res, device=device)
        seen.append((c.calls, c.uploads, c.sorts, c.copies))
    assert seen[0] == seen[1]
    calls, uploads, sorts, copies = seen[0]
    assert uploads == 1 and sorts == 1 and copies == 1
    assert calls == ["m2f_bits_pair_tiles", "m2f_rle_decode_bits_ragged", "m2f_poly_crossings",
                     "m2f_poly_decode_bits_ragged", "m2f_bits_pair_ragged_workspace", "m2f_bits_pair_counts_ragged"]


def test_a_batch_without_polygons_issues_the_calls_it_issues_today(device, monkeypatch):
    gt, results, _ = load_fixture()
    seen = []
    for kw in ({}, {"polygons": "rasterize"}):
        ground_truth = COCOGroundTruth(copy.deepcopy(gt), **kw)
        with monkeypatch.context() as mp:
            c = _Counter(mp)
            r = evaluate_coco(ground_truth, results, device=device)
        seen.append((c.calls, c.uploads, c.sorts, c.copies, r.stats.tolist()))
    assert seen[0] == seen[1]
    assert seen[0][0] == ["m2f_bits_pair_tiles", "m2f_rle_decode_bits_ragged", "m2f_bits_pair_ragged_workspace",
                          "m2f_bits_pair_counts_ragged"]
    assert seen[0][1:4] == (1, 0, 1)
