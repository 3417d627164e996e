"""The bodies test_boundary_cpu.py and test_boundary_gpu.py share: each takes the device the planes live on, so the numpy
restatement and the kernel answer to the same assertions.  Every comparison is bit or integer equality."""
import copy

import numpy as np
import pytest
import torch

import boundary_ref
from bm2f_amd import (COCOEvaluator, COCOGroundTruth, COCOParams, boundary_bits_ragged, boundary_dilation,
                      evaluate_coco, mask_pair_counts_ragged, mask_to_boundary_bits)
from boundary_cases import CASES, D_MAX, check_planes, expected, pack_batch, pack_plane, planes_of, run_ragged
from boundary_eval_cases import CONFIGS
from coco_eval_cases import FIELDS, flatten

GROUPS = {"grid": [i for i, c in enumerate(CASES) if c[0].startswith("grid")],
          "contents": [i for i, c in enumerate(CASES) if not c[0].startswith("grid")]}


def one_ragged_batch(device, group):
    """All cases of a group in one batch, each with its own d, tail bits and padding words set to ones."""
    idx = GROUPS[group]
    got, offsets, sizes = run_ragged(idx, device)
    check_planes(got, offsets, sizes, idx)
    covered = np.zeros(got.size, dtype=bool)
    for o, (H, W) in zip(offsets, sizes):
        covered[o:o + H * ((W + 31) // 32)] = True
    return got, covered


def full_mask_is_a_frame(device):
    for d in (1, 33, D_MAX):
        i = next(k for k, c in enumerate(CASES) if c[0] == f"full-d{d}")
        H, W = CASES[i][1].shape
        frame = np.ones((H, W), dtype=bool)
        frame[d:H - d, d:W - d] = False
        got, offsets, sizes = run_ragged([i], device)
        assert np.array_equal(planes_of(got, offsets, sizes)[0], pack_plane(frame, hostile=False))


def each_case_alone_and_packed(device):
    """A case alone gives the plane it gives inside the batch; planes packed back to back (offsets off the 4-word
    grid) and clean padding change nothing."""
    idx = GROUPS["grid"][::3] + GROUPS["contents"][::7]
    for i in idx:
        got, offsets, sizes = run_ragged([i], device)
        check_planes(got, offsets, sizes, [i])
    for kw in ({"align": 1}, {"hostile": False}):
        got, offsets, sizes = run_ragged(idx, device, **kw)
        check_planes(got, offsets, sizes, idx)
    assert any(o % 4 for o in pack_batch([CASES[i][1] for i in idx], align=1)[1])


def ratio_derived_dilation(device):
    """Every shape with d from the ratio: the default 0.02 gives d = 1 .. 16 on these sizes, 0.15 crosses 32."""
    idx = GROUPS["grid"] + GROUPS["contents"][::5]
    masks = [CASES[i][1] for i in idx]
    words, offsets, sizes = pack_batch(masks)
    for ratio in (0.02, 0.15):
        d = [boundary_ref.dilation(H, W, ratio) for H, W in sizes]
        assert d == [boundary_dilation(H, W, ratio) for H, W in sizes] and max(d) <= D_MAX
        kw = {} if ratio == 0.02 else {"dilation_ratio": ratio}
        got = boundary_bits_ragged(torch.from_numpy(words).to(device), offsets, sizes, **kw).cpu().numpy()
        check_planes(got, offsets, sizes, idx, dilations=d)
    assert max(d) >= 32


def ragged_and_uniform_agree(device):
    by_shape = {}
    for i, (_, m, d) in enumerate(CASES):
        by_shape.setdefault((m.shape, d), []).append(i)
    shapes = [k for k, v in by_shape.items() if len(v) >= 4]
    assert len(shapes) >= 8
    for (H, W), d in shapes:
        idx = by_shape[(H, W), d]
        planes = np.stack([pack_plane(CASES[i][1]) for i in idx])   # tail bits set
        planes = torch.from_numpy(planes).to(device).view(2, -1, H, planes.shape[-1]) if len(idx) % 2 == 0 \
            else torch.from_numpy(planes).to(device)
        got = mask_to_boundary_bits(planes, W, dilation=d)
        assert got.shape == planes.shape and got.device == planes.device and got.dtype == torch.int32
        for i, plane in zip(idx, got.cpu().numpy().reshape(len(idx), H, -1)):
            assert np.array_equal(plane, expected(i)), CASES[i][0]
    # d from the ratio and the size
    H, W = CASES[GROUPS["contents"][0]][1].shape
    i = GROUPS["contents"][5]
    one = torch.from_numpy(pack_plane(CASES[i][1])).to(device)
    got = mask_to_boundary_bits(one, W).cpu().numpy()
    assert np.array_equal(got, expected(i, boundary_ref.dilation(H, W)))
    assert mask_to_boundary_bits(torch.zeros((0, H, one.shape[-1]), dtype=torch.int32, device=device), W).shape[0] == 0


def pair_counts_on_boundaries(device):
    """m2f_bits_pair_counts_ragged, unchanged, on the boundary planes: the dense integer counts of the boundaries."""
    by_shape = {}
    for i, (_, m, d) in enumerate(CASES):
        by_shape.setdefault((m.shape, d), []).append(i)
    shapes = [k for k, v in by_shape.items() if len(v) >= 4][:6]
    idx = [i for k in shapes for i in by_shape[k]]
    words, offsets, sizes = pack_batch([CASES[i][1] for i in idx])
    out = boundary_bits_ragged(torch.from_numpy(words).to(device), offsets, sizes, dilations=[CASES[i][2] for i in idx])
    groups, at = [], 0
    for k in shapes:
        n = len(by_shape[k])
        groups.append((k[0][0], k[0][1], offsets[at:at + n - 2], offsets[at + n - 2:at + n]))
        at += n
    got = mask_pair_counts_ragged(out, groups)
    at = 0
    for k, (inter, area_a, area_b) in zip(shapes, got):
        dense = [boundary_ref.boundary(CASES[i][1], CASES[i][2], boundary_ref.erode_window) for i in by_shape[k]]
        a, b = np.stack(dense[:-2]), np.stack(dense[-2:])
        assert np.array_equal(inter, (a[:, None] & b[None]).sum((2, 3)))
        assert np.array_equal(area_a, a.sum((1, 2))) and np.array_equal(area_b, b.sum((1, 2)))


def refusals(device):
    """ValueError before any launch."""
    words, offsets, sizes = pack_batch([CASES[0][1], CASES[1][1]])
    t = torch.from_numpy(words).to(device)
    for d in (0, -1, D_MAX + 1, [1, D_MAX + 1]):
        with pytest.raises(ValueError, match="dilation"):
            boundary_bits_ragged(t, offsets, sizes, dilations=d)
    with pytest.raises(ValueError, match="dilation"):
        boundary_bits_ragged(t, offsets, sizes, dilation_ratio=1e6)
    for bad in (t.long(), t.float(), t.view(1, -1), words):
        with pytest.raises(ValueError, match="int32"):
            boundary_bits_ragged(bad, offsets, sizes)
    with pytest.raises(ValueError, match="integers"):
        boundary_bits_ragged(t, offsets, sizes, dilations=[1.0, 2.0])
    with pytest.raises(ValueError):
        boundary_bits_ragged(t, offsets, sizes, dilations=[1, 2, 3])
    with pytest.raises(ValueError, match="fit"):
        boundary_bits_ragged(t, offsets + t.numel(), sizes)
    with pytest.raises(ValueError, match="fit"):
        boundary_bits_ragged(t, [-1, 0], sizes)
    with pytest.raises(ValueError, match="fit"):
        boundary_bits_ragged(t[:offsets[1]].clone(), offsets, sizes)     # the last plane ends behind the buffer
    with pytest.raises(ValueError):
        boundary_bits_ragged(t, offsets, sizes[:1])
    with pytest.raises(ValueError):
        boundary_bits_ragged(t, offsets, [(0, 5), (3, 3)])
    with pytest.raises(ValueError):
        mask_to_boundary_bits(t.view(1, -1), 40)                      # 40 columns are two words, not numel
    with pytest.raises(ValueError, match="dilation"):
        mask_to_boundary_bits(torch.zeros((2, 3, 1), dtype=torch.int32, device=device), 20, dilation=D_MAX + 1)
    assert boundary_bits_ragged(t, [], np.zeros((0, 2))).shape == t.shape


def flat(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, len(r.params.iouThrs))


def run_config(fixture, name, device=None, **kw):
    gt, results, _ = fixture
    max_dets, iou_type, ratio = CONFIGS[name]
    p = COCOParams(iou_type)
    p.maxDets = list(max_dets)
    if ratio is not None:
        kw["dilation_ratio"] = ratio
    return evaluate_coco(COCOGroundTruth(copy.deepcopy(gt)), copy.deepcopy(results), iou_type=iou_type, params=p,
                         device=device, **kw)


def assert_matches(got, want):
    """Exact, as in test_coco_eval_*: the IoUs are ratios of the same integers and the summary runs the same numpy
    operations in the same order as the oracle."""
    for f in FIELDS:
        assert got[f].shape == want[f].shape, f
        assert np.array_equal(got[f], want[f]), f


def evaluator_reports_boundary(fixture, device=None):
    gt, results, expected_eval = fixture
    names = [c["name"] for c in gt["categories"]]
    ev = COCOEvaluator(copy.deepcopy(gt), class_names=names, tasks=("segm", "boundary"), device=device)
    ev._predictions.extend(copy.deepcopy(results))
    m = ev.evaluate()
    assert set(m) == {"segm", "boundary"} and set(m["boundary"]) == set(m["segm"])
    assert m["boundary"]["AP"] == expected_eval["boundary"]["stats"][0] * 100
    assert m["segm"]["AP"] == expected_eval["segm"]["stats"][0] * 100
    wide = COCOEvaluator(copy.deepcopy(gt), tasks=("boundary",), dilation_ratio=CONFIGS["wide"][2], device=device)
    wide._predictions.extend(copy.deepcopy(results))
    assert wide.evaluate()["boundary"]["AP"] == expected_eval["wide"]["stats"][0] * 100
