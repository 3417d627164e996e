"""The instance and video-instance mappers on CPU tensors against the dense route of the same commit
(tests/instance_mapper_checks.py).  Every comparison is equality."""
import pytest

import instance_mapper_checks as checks

CPU = "cpu"


@pytest.mark.parametrize("form", ["rle", "mixed", "array"])
def test_decoded_route_equals_the_dense_route(form):
    checks.rle_route_equals_dense(CPU, form)


def test_polygon_route_equals_polygons_to_bits_of_the_moved_vertices():
    checks.polygon_route(CPU)


def test_mixed_routes_keep_annotation_order():
    checks.mixed_routes_keep_annotation_order(CPU)


def test_lsj_filter_drops_exactly_the_degenerate_rows():
    checks.lsj_filters_degenerate_rows(CPU)


def test_sample_clip_frames():
    checks.sample_clip_frames_rule()


def test_video_dummies_ids_and_targets():
    checks.video_dummies_and_ids(CPU)


def test_video_weaksup_targets_take_the_output_unchanged():
    checks.video_weaksup_targets(CPU)


def test_mappers_are_exported():
    import bm2f_amd
    for name in ("InstanceTrainMapper", "COCOInstanceLSJMapper", "VideoInstanceTrainMapper", "sample_clip_frames",
                 "instance_views", "bit_boxes_ragged"):
        assert hasattr(bm2f_amd, name), name
