"""The instance and video-instance mappers on the device against the dense route of the same commit
(tests/instance_mapper_checks.py), and their outputs through the target preparations and one criterion forward.
Every comparison is equality."""
import pytest
import torch

import instance_mapper_checks as checks
import label_target_cases as ltc
from bm2f_amd.weaksup import prepare_weaksup_targets

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", ["rle", "mixed", "array"])
def test_decoded_route_equals_the_dense_route(form, device):
    checks.rle_route_equals_dense(device, form)


def test_polygon_route_equals_polygons_to_bits_of_the_moved_vertices(device):
    checks.polygon_route(device)


def test_mixed_routes_keep_annotation_order(device):
    checks.mixed_routes_keep_annotation_order(device)


def test_lsj_filter_drops_exactly_the_degenerate_rows(device):
    checks.lsj_filters_degenerate_rows(device)


def test_video_dummies_ids_and_targets(device):
    checks.video_dummies_and_ids(device)


def test_video_weaksup_targets_take_the_output_unchanged(device):
    checks.video_weaksup_targets(device)


def dense_targets(res, smp, device):
    out = []
    for i, t in enumerate(res["instances"]):
        masks = checks.samples("cpu", "rle")[1][i]
        m, b = checks.dense_route(masks, res["views"][i], device)
        out.append({"labels": t["labels"].clone(), "masks": m, "boxes": b})
    return out


def test_weaksup_targets_and_criterion_take_the_output_unchanged(device):
    res, smp = checks.rle_route_equals_dense(device, "rle")
    want_t = dense_targets(res, smp, device)
    org = [res["images"][i].float() for i in range(3)]
    got = prepare_weaksup_targets(res["instances"], org, [64, 64, 64])
    want = prepare_weaksup_targets(want_t, org, [64, 64, 64])
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # one mask-supervised criterion forward: the mapper's dicts against the dense-route dicts, float masks as the
    # reference's prepare_targets makes them
    _, _, heads = ltc.criterion_case()
    as_float = lambda ts: [{"labels": t["labels"], "masks": t["masks"].float()} for t in ts]   # noqa: E731
    la, seen_a, _ = ltc.run_criterion(device, as_float(res["instances"]), heads)
    lb, seen_b, _ = ltc.run_criterion(device, as_float(want_t), heads)
    assert la.keys() == lb.keys()
    for ia, ib in zip(seen_a, seen_b):
        for (qa, ta), (qb, tb) in zip(ia, ib):
            assert torch.equal(torch.as_tensor(qa), torch.as_tensor(qb))
            assert torch.equal(torch.as_tensor(ta), torch.as_tensor(tb))
    for k in la:
        ltc.same_loss(k, la[k], lb[k], bitwise=True)
