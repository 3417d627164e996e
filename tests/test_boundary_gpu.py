"""``m2f_bits_boundary_ragged`` (csrc/mask_boundary.hip) on the device against the dense oracles of
tests/boundary_ref.py, bit for bit, on the cases of tests/boundary_cases.py, and Boundary AP on the device against its
CPU run and the fixtures.  Every comparison is bit or integer equality."""
import copy

import numpy as np
import pytest
import torch

import boundary_checks as checks
from bm2f_amd import COCOGroundTruth, _native, convert_polygons_to_rle, evaluate_coco, rle_encode
from bm2f_amd.mask_boundary import boundary_pair_counts_ragged
from boundary_cases import CASES
from boundary_eval_cases import CONFIGS, load_fixture
from coco_eval_cases import FIELDS
from polygon_cases import polygon_ground_truth

pytestmark = pytest.mark.gpu

FIXTURE = load_fixture()


@pytest.mark.parametrize("group", list(checks.GROUPS))
def test_one_ragged_batch_equals_the_oracle(group, device):
    """Hostile padding: the words between the output's planes are unspecified, the planes are exact."""
    checks.one_ragged_batch(device, group)


def test_full_mask_is_a_frame(device):
    checks.full_mask_is_a_frame(device)


def test_each_case_alone_and_packed(device):
    checks.each_case_alone_and_packed(device)


def test_ratio_derived_dilation(device):
    checks.ratio_derived_dilation(device)


def test_ragged_and_uniform_agree(device):
    checks.ragged_and_uniform_agree(device)


def test_pair_counts_on_boundaries(device):
    checks.pair_counts_on_boundaries(device)


def test_refusals_come_before_any_launch(device, monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: calls.append(name) or real(name, *a))
    checks.refusals(device)
    assert "m2f_bits_boundary_ragged" not in calls


def test_device_planes_equal_the_cpu_planes(device):
    """The kernel and the numpy restatement on the same hostile buffer, plane by plane."""
    idx = list(range(0, len(CASES), 2))
    got, offsets, sizes = checks.run_ragged(idx, device)
    cpu, _, _ = checks.run_ragged(idx, torch.device("cpu"))
    for g, c in zip(checks.planes_of(got, offsets, sizes), checks.planes_of(cpu, offsets, sizes)):
        assert np.array_equal(g, c)


def _same(x, y):
    return len(x) == len(y) and all(p.dtype == np.int64 and p.shape == q.shape and np.array_equal(p, q)
                                    for gx, gy in zip(x, y) for p, q in zip(gx, gy))


def test_batch_step_on_device_equals_cpu(device):
    """The evaluator's batch step, masks of three sizes with a None plane and an empty group side: both count
    triples equal the CPU path's.  Not replayed as a graph."""
    idx = checks.GROUPS["contents"][:5] + checks.GROUPS["grid"][20:23] + checks.GROUPS["contents"][-4:]
    rles = [rle_encode(torch.from_numpy(CASES[i][1])[None])[0] for i in idx] + [None]
    shape = [CASES[i][1].shape for i in idx]
    sizes = [None] * len(idx) + [shape[0]]
    groups = [(*shape[0], [0, 1, 2, 12], [3, 4]), (*shape[5], [5], []), (*shape[6], [], [6]), (*shape[7], [7], [7]),
              (*shape[8], [8, 9, 10], [11])]
    got = boundary_pair_counts_ragged(rles, groups, device=device, sizes=sizes)
    want = boundary_pair_counts_ragged(rles, groups, sizes=sizes)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert got[1][0][1].sum() > 0 and (got[1][0][1] <= got[0][0][1]).all()      # a boundary is part of its mask


@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c[1] == "boundary"])
def test_evaluate_coco_on_device_equals_cpu_and_oracle(name, device):
    cpu = checks.flat(checks.run_config(FIXTURE, name))
    for kw in ({}, {"batch_bytes": 600_000}, {"batch_bytes": 1}):
        got = checks.flat(checks.run_config(FIXTURE, name, device=device, **kw))
        for f in FIELDS:
            assert np.array_equal(got[f], cpu[f]), (f, kw)
            assert np.array_equal(got[f], FIXTURE[2][name][f]), (f, kw)


def test_evaluator_reports_boundary(device):
    checks.evaluator_reports_boundary(FIXTURE, device=device)


def test_polygon_ground_truth_rasterized_equals_the_converted_file(device):
    poly_gt, _, results = polygon_ground_truth()
    converted = convert_polygons_to_rle(poly_gt)
    want = checks.flat(evaluate_coco(COCOGroundTruth(converted), results, iou_type="boundary"))
    for kw in ({}, {"batch_bytes": 300_000}):
        gt = COCOGroundTruth(copy.deepcopy(poly_gt), polygons="rasterize")
        got = checks.flat(evaluate_coco(gt, results, iou_type="boundary", device=device, **kw))
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), (f, kw)
    segm = checks.flat(evaluate_coco(COCOGroundTruth(converted), results))
    assert not np.array_equal(segm["iou_values"], want["iou_values"])


def test_launches_and_copies_do_not_grow_with_the_batch(device, monkeypatch):
    gt, results, _ = FIXTURE
    seen = []
    for images in ({1, 10}, {1, 5, 6, 7, 8, 10, 11, 12}):
        sub = copy.deepcopy(gt)
        sub["images"] = [im for im in sub["images"] if im["id"] in images]
        sub["annotations"] = [a for a in sub["annotations"] if a["image_id"] in images]
        res = [r for r in results if r["image_id"] in images]
        calls, counts = [], {"uploads": 0, "copies": 0}
        with monkeypatch.context() as mp:
            real_call, real_upload, real_cpu = _native.call, _native.upload_tables, torch.Tensor.cpu
            mp.setattr(_native, "call", lambda name, *a: calls.append(name) or real_call(name, *a))

            def upload(tables, dev):
                counts["uploads"] += 1
                return real_upload(tables, dev)

            def cpu(t, *a, **k):
                counts["copies"] += t.device.type == "cuda"
                return real_cpu(t, *a, **k)
            mp.setattr(_native, "upload_tables", upload)
            mp.setattr(torch.Tensor, "cpu", cpu)
            evaluate_coco(COCOGroundTruth(sub), res, iou_type="boundary", device=device)
        seen.append((calls, counts["uploads"], counts["copies"]))
    assert seen[0] == seen[1]
    calls, uploads, copies = seen[0]
    assert uploads == 1 and copies == 1
    launches = [c for c in calls if not c.endswith("_tiles") and not c.endswith("_workspace")]
    assert launches == ["m2f_rle_decode_bits_ragged", "m2f_bits_boundary_ragged", "m2f_bits_pair_counts_ragged",
                        "m2f_bits_pair_counts_ragged"]
