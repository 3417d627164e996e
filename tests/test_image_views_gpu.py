"""``m2f_image_views`` and ``m2f_label_views`` (csrc/image_views.hip) on the device against Pillow's recorded outputs
(tests/golden/image_views.npz) and against the CPU definition, on the cases of tests/image_view_cases.py.  Every
comparison is exact equality."""
import importlib

import numpy as np
import pytest
import torch

import image_view_cases as ivc
import image_view_checks as checks
from bm2f_amd import _native

pytestmark = pytest.mark.gpu

mod = importlib.import_module("bm2f_amd.image_views")
CPU = torch.device("cpu")


@pytest.mark.parametrize("case", ivc.IMAGE_CASES, ids=lambda c: c["name"])
def test_image_case_equals_the_fixture_and_the_cpu_path(case, device):
    checks.image_case(case, device, expected=checks.run_image(case, CPU)[0].numpy())


@pytest.mark.parametrize("dtype", list(ivc.LABEL_DTYPES))
def test_label_cases_equal_the_fixture_and_the_cpu_path(dtype, device):
    for case in ivc.LABEL_CASES:
        if case["dtype"] == dtype:
            checks.label_case(case, device, expected=checks.run_label(case, CPU)[0].numpy())
    checks.label_batch_pad(device)


def test_ragged_batch_writes_every_element(device):
    checks.ragged_batch(device)


def test_output_dtypes(device):
    checks.output_dtypes(device)


def test_all_cases_in_one_launch_equal_the_cpu_path(device):
    """Every image case as one ragged call of one launch: the views' tables and tile heights share a launch."""
    srcs = [torch.from_numpy(ivc.image_source(c)) for c in ivc.IMAGE_CASES]
    views = [checks.view_of(c, i) for i, c in enumerate(ivc.IMAGE_CASES)]
    want, wsizes = mod.image_views(srcs, views, out_dtype=torch.uint8, size_divisibility=32, pad_value=3)
    got, gsizes = mod.image_views([s.to(device) for s in srcs], views, out_dtype=torch.uint8, size_divisibility=32,
                                  pad_value=3)
    assert gsizes == wsizes and torch.equal(got.cpu(), want)


def test_refusals_come_before_any_launch(device, monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: calls.append(name) or real(name, *a))
    checks.refusals(device)
    assert calls == ["m2f_image_views"]                      # the admitted 64x view at the end of the check


def test_bad_table_row_is_status_3_and_nothing_is_written(device):
    """A row that points outside the source range: M2F_EUNSUPPORTED from the host check, the output untouched."""
    img = torch.from_numpy(ivc.image_source(ivc.IMAGE_BY_NAME["pair1"])).to(device)
    plan = mod._Plan([mod.View(size=(19, 23))], [tuple(img.shape[:2])], image=True)
    for column, value in ((0, 1), (3, 3 * 53 + 1), (1, 38), (14, 1 << 40), (10, 20), (4, 0)):
        rows = plan.rows.copy()
        rows[0, 3] = 3 * 53
        rows[0, column] = value
        out = torch.full((1, 3, 19, 23), 0xA5, dtype=torch.uint8, device=device)
        with pytest.raises(_native.NativeError, match=r"code 3\).*view 0"):
            mod._launch_image(img.data_ptr(), img.numel(), plan, rows, out, None, None, 0.0)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()), column
    lab = torch.zeros(1, 37, 53, dtype=torch.int16, device=device)
    plan = mod._Plan([mod.View(size=(19, 23))], [(37, 53)], image=False)
    rows = plan.rows.copy()
    rows[0, 3], rows[0, 17] = 53, 37 * 53
    rows[0, 0] = 2
    out = torch.full((1, 1, 19, 23), 0x5A5A, dtype=torch.int16, device=device)
    with pytest.raises(_native.NativeError, match=r"code 3\).*view 0"):
        mod._launch_label(lab.data_ptr(), 2, lab.numel(), plan, rows, out)
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())


def test_tta_mapper(device):
    checks.tta_mapper(device)


def test_tta_mapper_is_one_launch(device, monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: calls.append(name) or real(name, *a))
    img = torch.from_numpy(ivc.tta_image()).permute(2, 0, 1).contiguous()
    mod.DeviceTTAMapper(ivc.TTA["min_sizes"], ivc.TTA["max_size"], device=device)({"image": img})
    assert calls == ["m2f_image_views"]


def test_preprocess_test_images(device):
    checks.preprocess(device)


def test_resize_image(device):
    checks.resize_image_is_one_view(device)
