"""Label-map RLE on the device: the kernels of csrc/label_rle.hip against the host definition, string for string and
integer for integer, the painter kernel against the planes, the public pieces on the device, and the error codes of
the new C entry points.  The cases are those of tests/label_rle_cases.py; every comparison is equality."""
import ctypes

import pytest
import torch

import label_rle_cases as lc
from bm2f_amd import _native, label_maps_to_rle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(lc.CASES))
def test_device_equals_definition(device, name):
    planes, kw = lc.CASES[name]
    dev_planes = lc.to_device(planes, device)
    assert [p.stride() for p in dev_planes] == [p.stride() for p in planes]      # a crop view is read in place
    got = label_maps_to_rle(dev_planes, **kw)
    assert got == lc.definition(name)
    assert label_maps_to_rle(dev_planes, **kw) == got                            # the same bytes on every run


@pytest.mark.parametrize("name", list(lc.CASES))
def test_paint_inverts_encode(device, name):
    got, want = lc.painted_back(name, device)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.device.type == "cuda" and g.dtype == w.dtype and torch.equal(g.cpu(), w)


def test_two_copies_per_call(device, monkeypatch):
    """The host receives the run totals and then one buffer of headers, offsets and bytes: no map, no mask."""
    planes, kw = lc.CASES["batch_scalar_ignore"]
    dev_planes = lc.to_device(planes, device)
    moved = []
    orig = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (moved.append(t.numel() * t.element_size()),
                                                                 orig(t, *a, **k))[1])
    label_maps_to_rle(dev_planes, **kw)
    assert len(moved) == 2 and moved[0] == 8 * (len(planes) + 1)


def test_painter(device):
    lc.check_painter(device)


def test_sem_seg_json_round_trip(device):
    lc.check_sem_seg_json(device)


def test_evaluator_keeps_and_writes_predictions(device, tmp_path):
    lc.check_evaluator(device, tmp_path)


def test_tool_prints_the_evaluator_metrics(device, tmp_path):
    lc.check_tool(device, tmp_path)


def test_panoptic_to_coco_detection(device):
    lc.check_panoptic_to_detection(device)


def test_instance_map_annotations(device):
    lc.check_instance_map(device)


def test_errors(device):
    lc.check_errors(device)


_P = ctypes.c_void_p(1 << 20)    # aligned, non-null, never dereferenced: every call below returns before the device
# entry point -> (valid-looking arguments, the positions of its pointers, the positions of its sizes)
_ENTRY_POINTS = {
    "m2f_label_rle_col_counts": ([_P, 1, 1, 1, _P, 8, None], (0, 4), (2, 5)),
    "m2f_label_rle_runs": ([_P, 1, 1, 1, _P, 8, _P, _P, 8, None], (0, 4, 6, 7), (2, 5, 8)),
    "m2f_label_rle_spans": ([_P, _P, 8, _P, _P, _P, 1, None, None, 4, _P, _P, _P, _P, None],
                            (0, 1, 3, 4, 5, 10, 11, 12, 13), (2, 9)),
    "m2f_label_rle_seg_keys": ([_P, _P, _P, 8, _P, 4, _P, None], (0, 1, 2, 4, 6), (3, 5)),
    "m2f_label_rle_segments": ([_P, 8, _P, _P, _P, _P, _P, 1, _P, _P, 4, _P, 16, _P, _P, None],
                               (0, 2, 3, 4, 5, 6, 8, 9, 11, 13, 14), (1, 10, 12)),
    "m2f_rle_paint_labels": ([_P, 8, _P, 1, _P, _P, 1, 1, 0, 1, _P, 8, None], (0, 2, 4, 5, 10), (1, 3, 7, 11)),
}
_DTYPE_ARG = {"m2f_label_rle_col_counts": 3, "m2f_label_rle_runs": 3, "m2f_rle_paint_labels": 9}


@pytest.mark.parametrize("name", sorted(_ENTRY_POINTS))
def test_entry_points_refuse_bad_arguments(device, name):
    """A null pointer, a negative size and an unknown dtype give M2F_EINVAL before any HIP call."""
    lib = _native.load()
    args, pointers, sizes = _ENTRY_POINTS[name]
    for at in pointers:
        bad = list(args)
        bad[at] = None
        assert getattr(lib, name)(*bad) == 1, (name, at)
        assert b"null pointer" in lib.m2f_last_error()
    for at in sizes:
        bad = list(args)
        bad[at] = -1
        assert getattr(lib, name)(*bad) == 1, (name, at)
        assert b"sizes must be positive" in lib.m2f_last_error()
    if name in _DTYPE_ARG:
        bad = list(args)
        bad[_DTYPE_ARG[name]] = 3
        assert getattr(lib, name)(*bad) == 1
        assert b"dtype 3" in lib.m2f_last_error()
