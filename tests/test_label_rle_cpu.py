"""Label-map RLE on the host: the definition of label_maps_to_rle against the literal per-value loop
(rle_encode(plane == v), numpy count and box), the painter against the planes, and the public pieces that hang on
them.  The cases are those of tests/label_rle_cases.py; every comparison is equality."""
import pytest
import torch

import label_rle_cases as lc
from bm2f_amd import label_maps_to_rle, rle_decode, string_to_counts


@pytest.mark.parametrize("name", list(lc.CASES))
def test_definition_equals_literal_loop(name):
    planes, kw = lc.CASES[name]
    assert lc.definition(name) == lc.literal(planes, **kw)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_paint_inverts_encode(name):
    got, want = lc.painted_back(name, "cpu")
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)


def test_extremes_are_what_they_claim():
    """The cases named after a property have it."""
    one, = lc.definition("one_label")
    assert len(one) == 1 and string_to_counts(one[0]["segmentation"]["counts"]) == [0, 360]
    seg = {e["label"]: e for e in lc.definition("owns_pixel0")[0]}[3]
    assert string_to_counts(seg["segmentation"]["counts"]) == [0, 1, 359]
    seg = {e["label"]: e for e in lc.definition("last_run_ends_at_HW")[0]}[4]
    assert string_to_counts(seg["segmentation"]["counts"]) == [359, 1]
    seg = {e["label"]: e for e in lc.definition("run_crosses_columns")[0]}[2]
    counts = string_to_counts(seg["segmentation"]["counts"])
    assert 4 in counts[1::2] and seg["bbox"] == [5, 0, 28, 9]             # rows 7, 8 of column 31 + rows 0, 1 of 32
    assert lc.definition("batch_scalar_ignore")[1] == [] and lc.definition("batch_per_image_ignore")[1] == []
    assert lc.definition("batch_with_empty_plane")[1] == []
    assert len(lc.definition("40x40_every_pixel")[0]) == 1600
    assert [e["label"] for e in lc.definition("int32_signed")[0]] == [-2 ** 31, -1, 0, 2 ** 24 + 5, 2 ** 31 - 1]
    big, = lc.definition("1056x1000_one_label")[0]
    assert len(big["segmentation"]["counts"]) == 1 + 5 and big["area"] == 1056000 and big["bbox"] == [0, 0, 1000, 1056]
    absent = lc.definition("ids_absent")[0]
    assert [e["label"] for e in absent] == [1, 33, 300, -4, 17] and [e["area"] for e in absent[1:4]] == [0, 0, 0]
    assert not rle_decode(absent[1]["segmentation"]).any() and absent[1]["bbox"] == [0, 0, 0, 0]
    assert label_maps_to_rle([]) == []


def test_painter():
    lc.check_painter("cpu")


def test_sem_seg_json_round_trip():
    lc.check_sem_seg_json("cpu")


def test_evaluator_keeps_and_writes_predictions(tmp_path):
    lc.check_evaluator(None, tmp_path)


def test_tool_prints_the_evaluator_metrics(tmp_path):
    lc.check_tool("cpu", tmp_path)


def test_panoptic_to_coco_detection():
    lc.check_panoptic_to_detection("cpu")


def test_instance_map_annotations():
    lc.check_instance_map("cpu")


def test_errors():
    lc.check_errors("cpu")
