"""bm2f_amd.image_views on CPU tensors (the numpy / torch definition) against Pillow: the recorded outputs of
tests/golden/image_views.npz always, and Pillow itself where it is installed.  Every comparison is exact equality."""
import importlib

import numpy as np
import pytest
import torch

import image_view_cases as ivc
import image_view_checks as checks
from bm2f_amd import View, lsj_view, resize_shortest_edge_size

mod = importlib.import_module("bm2f_amd.image_views")
CPU = torch.device("cpu")


@pytest.mark.parametrize("case", ivc.IMAGE_CASES, ids=lambda c: c["name"])
def test_image_case_equals_the_fixture(case):
    checks.image_case(case, CPU)


@pytest.mark.parametrize("dtype", list(ivc.LABEL_DTYPES))
def test_label_cases_equal_the_fixture(dtype):
    for case in ivc.LABEL_CASES:
        if case["dtype"] == dtype:
            checks.label_case(case, CPU)
    checks.label_batch_pad(CPU)


def test_cases_equal_pillow_live():
    pytest.importorskip("PIL")
    for case in ivc.IMAGE_CASES:
        checks.image_case(case, CPU, expected=ivc.pil_image(case))
    for case in ivc.LABEL_CASES:
        checks.label_case(case, CPU, expected=ivc.pil_label(case))


def test_more_shape_pairs_equal_pillow_live():
    """Pairs too large for the fixture, images and label maps."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for (H, W), (h, w) in [((480, 640), (512, 683)), ((101, 77), (333, 20)), ((200, 3), (50, 9)), ((130, 70), (3, 2))]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        got = mod.resize_image(torch.from_numpy(img), (h, w)).permute(1, 2, 0).numpy()
        assert np.array_equal(got, np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR)))
        lab = rng.integers(0, 1 << 20, (H, W)).astype(np.int32)
        got, _ = mod.label_views([torch.from_numpy(lab)], [View(size=(h, w))], seg_pad=0)
        assert np.array_equal(got[0, 0].numpy(), np.asarray(Image.fromarray(lab, mode="I").resize((w, h), Image.NEAREST)))


def test_ragged_batch():
    checks.ragged_batch(CPU)


def test_output_dtypes():
    checks.output_dtypes(CPU)


def test_refusals():
    checks.refusals(CPU)


def test_tta_mapper():
    checks.tta_mapper(CPU)


def test_preprocess_test_images():
    checks.preprocess(CPU)


def test_resize_image():
    checks.resize_image_is_one_view(CPU)


def test_tables():
    """An axis that keeps its size has no table (PIL skips the pass); ksize and the bounds of a 2x reduction; the
    running sum of the nearest index differs from (x + 0.5) * a somewhere, which is why it is restated as a sum."""
    assert mod.bilinear_table(7, 7) is None
    bounds, coeffs = mod.bilinear_table(8, 4)
    assert coeffs.shape == (4, 5) and bounds.dtype == np.int32 and coeffs.dtype == np.int32
    assert bounds.tolist() == [[0, 3], [1, 4], [3, 4], [5, 3]]
    assert coeffs[1].tolist() == [1 << 19, 3 << 19, 3 << 19, 1 << 19, 0]
    assert mod.nearest_table(4, 8).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert mod.bilinear_table(8, 4) is mod.bilinear_table(8, 4)          # cached per (in, out)


def test_resize_shortest_edge_size_by_hand():
    # 480 x 640, size 512: scale 1.0667, long side 682.67 -> 683
    assert resize_shortest_edge_size(480, 640, 512, 2048) == (512, 683)
    # 500 x 1500, size 800, max 1333: (800, 2400) -> scale 1333 / 2400: (444.33, 1333) -> (444, 1333)
    assert resize_shortest_edge_size(500, 1500, 800, 1333) == (444, 1333)
    # 20 x 50, size 5: long side 12.5 -> int(13.0) = 13 (half rounds up here, not to even)
    assert resize_shortest_edge_size(20, 50, 5, 100) == (5, 13)


def test_lsj_view_by_hand():
    # 480 x 640 into 1024 at scale 0.5: target 512, r = min(512/480, 512/640) = 0.8 -> (384, 512); no offset room
    assert lsj_view(480, 640, 1024, 0.5, 0.7, False) == View(size=(384, 512), crop=(0, 0, 1024, 1024),
                                                              canvas=(1024, 1024), fill=128)
    # scale 2.0: target 2048, r = 3.2 -> (1536, 2048); offsets round(512 * 0.25) = 128, round(1024 * 0.25) = 256
    assert lsj_view(480, 640, 1024, 2.0, 0.25, True) == View(size=(1536, 2048), crop=(128, 256, 1024, 1024),
                                                              canvas=(1024, 1024), flip_in=True, fill=128)
    # 10 x 5 into 4 at scale 1.25: target 5, r = 0.5 -> (5, round-half-even(2.5) = 2); offset round(1 * 0.5) = 0 (even)
    assert lsj_view(10, 5, 4, 1.25, 0.5, False) == View(size=(5, 2), crop=(0, 0, 4, 4), canvas=(4, 4), fill=128)
