"""Boundary planes and Boundary AP on the host (no GPU): the two dense oracles of tests/boundary_ref.py against each
other, the numpy restatement of ``boundary_bits_ragged`` / ``mask_to_boundary_bits`` against them bit for bit on the
cases of tests/boundary_cases.py, the refusals, and ``evaluate_coco(iou_type="boundary")`` against fixtures whose
matching, accumulation and summary are the reference's YTVOSeval with a dense scipy min(mask IoU, boundary IoU)
(tests/golden/gen_boundary_eval_golden.py, which asserts what the data covers)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary_checks as checks
import boundary_ref
from bm2f_amd import COCOGroundTruth, _native, boundary_dilation, evaluate_coco
from bm2f_amd.mask_boundary import boundary_pair_counts_ragged, boundary_tiles
from boundary_cases import BAND, CASES, D_MAX, DILATIONS, HEIGHTS, TILE_WORDS, WIDTHS
from boundary_eval_cases import CONFIGS, GT_JSON, RESULTS_JSON, load_fixture
from conftest import ROOT

CPU = torch.device("cpu")
FIXTURE = load_fixture()


def test_the_two_oracles_agree_on_every_case():
    for name, mask, d in CASES:
        assert np.array_equal(boundary_ref.erode_scipy(mask, d), boundary_ref.erode_window(mask, d)), name
        r = boundary_ref.dilation(*mask.shape)
        assert np.array_equal(boundary_ref.erode_scipy(mask, r), boundary_ref.erode_window(mask, r)), name


def test_cases_cover_what_they_claim():
    assert (BAND, TILE_WORDS, D_MAX) == boundary_tiles() and D_MAX >= 128
    shapes = {c[1].shape for c in CASES}
    assert {h for h, _ in shapes} >= set(HEIGHTS) and {w for _, w in shapes} >= set(WIDTHS)
    assert {c[2] for c in CASES} == set(DILATIONS) and {1, 2, 3, 31, 32, 33, 64} <= set(DILATIONS)
    assert BAND + 1 in HEIGHTS and any(h > 2 * BAND for h in HEIGHTS) and any(w > 32 * TILE_WORDS for w in WIDTHS)
    for name, mask, d in CASES:
        e = boundary_ref.erode_window(mask, d)
        if name.startswith("thick2d-"):
            assert mask.any() and not e.any(), name                   # the boundary equals the mask
        if name.startswith("thick2d1-rows"):
            assert e.any(1).sum() == 1, name                          # one surviving row
        if name.startswith("thick2d1-cols"):
            assert e.any(0).sum() == 1, name
        if name.startswith("hole-"):
            full = boundary_ref.erode_window(np.ones_like(mask), d)
            assert (~mask).sum() <= d * d and full.sum() > e.sum(), name   # smaller than d, and it costs survivors
    assert boundary_dilation(1000, 1300) == 33 and boundary_dilation(480, 640) == 16 and boundary_dilation(5, 5) == 1
    assert boundary_dilation(300, 420, 0.05) == boundary_ref.dilation(300, 420, 0.05) == 26


@pytest.mark.parametrize("group", list(checks.GROUPS))
def test_one_ragged_batch_equals_the_oracle(group):
    got, covered = checks.one_ragged_batch(CPU, group)
    assert not got[~covered].any()                                    # the CPU path leaves zeros between planes


def test_full_mask_is_a_frame():
    checks.full_mask_is_a_frame(CPU)


def test_each_case_alone_and_packed():
    checks.each_case_alone_and_packed(CPU)


def test_ratio_derived_dilation():
    checks.ratio_derived_dilation(CPU)


def test_ragged_and_uniform_agree():
    checks.ragged_and_uniform_agree(CPU)


def test_pair_counts_on_boundaries():
    checks.pair_counts_on_boundaries(CPU)


def test_refusals():
    checks.refusals(CPU)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _native.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    L = ctypes.c_int64
    ok = (p, L(1024), 2, p, p, p, p, L(4), 16, q, None)
    for bad, text in ((dict({0: None}), b"null"), (dict({9: None}), b"null"), (dict({2: 0}), b"positive"),
                      (dict({8: 0}), b"max_dilation"), (dict({8: D_MAX + 1}), b"max_dilation"),
                      (dict({9: ctypes.c_void_p((1 << 20) + 64)}), b"overlap"),
                      (dict({4: ctypes.c_void_p((1 << 20) + 4)}), b"aligned")):
        args = [bad.get(i, a) for i, a in enumerate(ok)]
        assert lib.m2f_bits_boundary_ragged(*args) == 1 and text in lib.m2f_last_error(), text
    assert lib.m2f_bits_boundary_ragged(*ok[:1], L(1 << 31), *ok[2:]) == 3
    assert lib.m2f_bits_boundary_tiles(None, None, None) == 1


@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_coco_equals_oracle(name):
    checks.assert_matches(checks.flat(checks.run_config(FIXTURE, name)), FIXTURE[2][name])


def test_fixture_tells_boundary_from_segm():
    e = FIXTURE[2]
    assert e["boundary"]["stats"][0] > 0 and e["boundary"]["stats"][0] != e["segm"]["stats"][0]
    assert not np.array_equal(e["boundary"]["dtMatches"], e["segm"]["dtMatches"])
    assert not np.array_equal(e["wide"]["stats"], e["boundary"]["stats"])
    assert (e["boundary"]["iou_values"] <= e["segm"]["iou_values"]).all()   # a minimum with the mask IoU


def test_batch_size_does_not_change_the_result():
    whole = checks.flat(checks.run_config(FIXTURE, "boundary"))
    for batch_bytes in (1, 100_000, 1 << 20):
        checks.assert_matches(checks.flat(checks.run_config(FIXTURE, "boundary", batch_bytes=batch_bytes)), whole)


def test_boundary_batches_count_the_second_buffer(monkeypatch):
    """The boundary planes double a batch's bytes: the images are cut as "segm" cuts them at half the budget."""
    ce = importlib.import_module("bm2f_amd.coco_eval")
    seen = []
    real = ce.image_batches
    monkeypatch.setattr(ce, "image_batches", lambda *a: seen.append(real(*a)) or seen[-1])
    checks.run_config(FIXTURE, "boundary", batch_bytes=2_000_000)
    checks.run_config(FIXTURE, "segm", batch_bytes=1_000_000)
    checks.run_config(FIXTURE, "segm", batch_bytes=2_000_000)
    assert seen[0] == seen[1] and seen[0] != seen[2]


def test_bbox_fields_are_ignored_and_other_refusals_stay():
    gt, results, expected = FIXTURE
    nobox = [{k: v for k, v in r.items() if k != "bbox"} for r in results]
    r = evaluate_coco(COCOGroundTruth(gt), nobox, iou_type="boundary")
    assert np.array_equal(r.stats, expected["boundary"]["stats"])
    with pytest.raises(NotImplementedError):
        evaluate_coco(COCOGroundTruth(gt), results, iou_type="keypoints")
    p = checks.COCOParams("boundary")
    p.useCats = 0
    with pytest.raises(NotImplementedError):
        evaluate_coco(COCOGroundTruth(gt), results, iou_type="boundary", params=p)
    with pytest.raises(ValueError, match="dilation"):                 # d = 0.5 * diagonal is beyond the kernel's range
        evaluate_coco(COCOGroundTruth(gt), results, iou_type="boundary", dilation_ratio=0.5)


def test_evaluator_reports_boundary():
    checks.evaluator_reports_boundary(FIXTURE)


def test_batch_step_returns_both_counts():
    """boundary_pair_counts_ragged against dense counts of masks and boundaries, with a None plane."""
    idx = checks.GROUPS["contents"][:6]
    H, W = CASES[idx[0]][1].shape
    from bm2f_amd import rle_encode
    rles = [rle_encode(torch.from_numpy(CASES[i][1])[None])[0] for i in idx] + [None]
    sizes = [None] * len(idx) + [(H, W)]
    groups = [(H, W, [0, 1, 2, 6], [3, 4, 5])]
    (m_inter, m_a, m_b), = boundary_pair_counts_ragged(rles, groups, sizes=sizes)[0]
    (b_inter, b_a, b_b), = boundary_pair_counts_ragged(rles, groups, sizes=sizes)[1]
    d = boundary_ref.dilation(H, W)
    dense = [CASES[i][1] for i in idx] + [np.zeros((H, W), dtype=bool)]
    edge = [boundary_ref.boundary(m, d) for m in dense]
    for inter, aa, ab, planes in ((m_inter, m_a, m_b, dense), (b_inter, b_a, b_b, edge)):
        a, b = np.stack([planes[i] for i in (0, 1, 2, 6)]), np.stack([planes[i] for i in (3, 4, 5)])
        assert np.array_equal(inter, (a[:, None] & b[None]).sum((2, 3)))
        assert np.array_equal(aa, a.sum((1, 2))) and np.array_equal(ab, b.sum((1, 2)))
    assert boundary_pair_counts_ragged(rles, [], sizes=sizes) == ([], [])


def test_tool_prints_the_fixture_statistics(capsys):
    spec = importlib.util.spec_from_file_location("evaluate_coco_boundary_ap",
                                                  os.path.join(ROOT, "tools", "evaluate_coco_boundary_ap.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for argv, name in ((["--gt-json-file", GT_JSON, "--dt-json-file", RESULTS_JSON], "boundary"),
                       (["--gt-json-file", GT_JSON, "--dt-json-file", RESULTS_JSON, "--iou-type", "segm"], "segm"),
                       (["--gt-json-file", GT_JSON, "--dt-json-file", RESULTS_JSON, "--dilation-ratio", "0.05"],
                        "wide")):
        stats = tool.main(argv)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(" Average")]
        assert len(lines) == 12 and np.array_equal(stats, FIXTURE[2][name]["stats"])
        assert [float(ln.rsplit("=", 1)[1]) for ln in lines] == [float(f"{s:0.3f}") for s in stats]
        assert "IoU=0.50:0.95" in lines[0] and "IoU=0.50 " in lines[1] and "maxDets=  1" in lines[6]
