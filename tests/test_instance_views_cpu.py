"""instance_views on CPU tensors: the definition against Pillow (live, and the recorded fixture), the boxes and areas
against a literal restatement of BitMasks.get_bounding_boxes, and what is refused.  Every comparison is equality."""
import os

import numpy as np
import pytest
import torch

import instance_view_cases as ivc
from bm2f_amd.image_views import View
from bm2f_amd.instance_views import bit_boxes_ragged, instance_views

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_views.npz")


def run_case(case, out, device="cpu", garbage=None, **kw):
    masks = ivc.case_masks(case["hw"])
    words, offsets, sizes, view_of = ivc.ragged([masks], garbage)
    return instance_views(torch.from_numpy(words).to(device), offsets, sizes, view_of, [case["view"]], out=out, **kw)


def as_dense(masks, out, width):
    """The returned masks as (M, Hp, Wp) uint8; bit planes must have zero tail bits."""
    if out == "uint8":
        return masks.cpu().numpy()
    dense, clean = ivc.unpack(masks.cpu().numpy(), width)
    assert clean, "a tail bit is set"
    return dense


@pytest.mark.parametrize("out", ["bits", "uint8"])
@pytest.mark.parametrize("case", ivc.CASES, ids=lambda c: c["name"])
def test_definition_equals_pillow(case, out):
    pytest.importorskip("PIL")
    masks, boxes, areas, sizes = run_case(case, out)
    Hc, Wc = ivc.canvas_of(case["view"])
    assert sizes == [(Hc, Wc)]
    want = np.stack([ivc.pil_view(m, case["view"]) for m in ivc.case_masks(case["hw"])])
    got = as_dense(masks, out, Wc)
    assert got.shape == want.shape and np.array_equal(got, want)
    wb, wa = ivc.bitmask_boxes(want)
    assert boxes.dtype == torch.float32 and np.array_equal(boxes.numpy(), wb)
    assert np.array_equal(areas.numpy(), wa)


def test_golden_file_is_pillows_output():
    pytest.importorskip("PIL")
    store = np.load(GOLDEN)
    fresh = ivc.golden_store(ivc.pil_view)
    assert set(fresh) | {"pillow_version"} == set(store.files)
    for k, v in fresh.items():
        assert np.array_equal(store[k], v), k


@pytest.mark.parametrize("case", ivc.CASES, ids=lambda c: c["name"])
def test_definition_equals_golden(case):
    store = np.load(GOLDEN)
    Hc, Wc = ivc.canvas_of(case["view"])
    masks = run_case(case, "uint8")[0]
    assert np.array_equal(masks.numpy(), ivc.golden_masks(store, case["name"], (Hc, Wc)))


def test_empty_and_full_and_single_pixels():
    case = ivc.CASES[0]                                       # (40, 33) -> (80, 65), no crop
    _, boxes, areas, _ = run_case(case, "bits")
    k = {n: i for i, n in enumerate(ivc.KINDS)}
    assert boxes[k["empty"]].tolist() == [0, 0, 0, 0] and int(areas[k["empty"]]) == 0
    assert boxes[k["full"]].tolist() == [0, 0, 65, 80] and int(areas[k["full"]]) == 80 * 65
    assert boxes[k["first"]][:2].tolist() == [0, 0]
    assert boxes[k["last"]][2:].tolist() == [65, 80]


def test_garbage_tail_bits_and_padding_words_are_ignored():
    for case in ivc.CASES:
        clean = run_case(case, "bits")
        dirty = run_case(case, "bits", garbage=np.random.default_rng(5))
        for a, b in zip(clean[:3], dirty[:3]):
            assert torch.equal(a, b), case["name"]


def test_batch_with_0_1_and_70_instances():
    cases, lists = ivc.batch_masks()
    words, offsets, sizes, view_of = ivc.ragged(lists, np.random.default_rng(9))
    views = [c["view"] for c in cases]
    masks, boxes, areas, image_sizes = instance_views(torch.from_numpy(words), offsets, sizes, view_of, views,
                                                      size_divisibility=32, out="uint8")
    assert image_sizes == [ivc.canvas_of(v) for v in views]
    assert masks.shape == (77, 96, 96)
    store = np.load(GOLDEN)
    want = np.zeros((77, 96, 96), dtype=np.uint8)
    at = 0
    for i, (v, m) in enumerate(zip(views, lists)):
        if len(m):
            Hc, Wc = ivc.canvas_of(v)
            want[at:at + len(m), :Hc, :Wc] = ivc.golden_masks(store, f"batch{i}", (Hc, Wc))
            at += len(m)
    assert np.array_equal(masks.numpy(), want)
    wb, wa = ivc.bitmask_boxes(want)
    assert np.array_equal(boxes.numpy(), wb) and np.array_equal(areas.numpy(), wa)
    bits = instance_views(torch.from_numpy(words), offsets, sizes, view_of, views, size_divisibility=32)[0]
    assert bits.shape == (77, 96, 3) and np.array_equal(as_dense(bits, "bits", 96), want)


def test_bit_boxes_ragged_is_the_identity_view():
    a, b = ivc.case_masks((40, 33)), ivc.case_masks((17, 70))
    words, offsets, sizes, _ = ivc.ragged([a, b], np.random.default_rng(2))
    masks, boxes, areas = bit_boxes_ragged(torch.from_numpy(words), offsets, sizes, out="uint8")
    want = np.zeros((12, 40, 70), dtype=np.uint8)
    want[:6, :, :33], want[6:, :17, :] = a, b
    assert np.array_equal(masks.numpy(), want)
    wb, wa = ivc.bitmask_boxes(want)
    assert np.array_equal(boxes.numpy(), wb) and np.array_equal(areas.numpy(), wa)


def test_into_is_overwritten():
    case = ivc.CASES[6]
    into = torch.full((6, 64, 3), -1, dtype=torch.int32)
    masks = run_case(case, "bits", into=into)[0]
    assert masks is into and torch.equal(masks, run_case(case, "bits")[0])


def test_bad_tables_raise():
    masks = ivc.case_masks((40, 33))
    words, offsets, sizes, view_of = ivc.ragged([masks])
    w, view = torch.from_numpy(words), [View(size=(20, 20))]
    with pytest.raises(ValueError, match="does not fit"):
        instance_views(w, offsets + words.size, sizes, view_of, view)
    with pytest.raises(ValueError, match="does not fit"):
        instance_views(w, offsets - 1000, sizes, view_of, view)
    with pytest.raises(ValueError, match="positive"):
        instance_views(w, offsets, sizes * np.array([[1, 0]]), view_of, view)
    with pytest.raises(ValueError, match="positive"):
        instance_views(w, offsets, sizes * np.array([[-1, 1]]), view_of, view)
    with pytest.raises(ValueError, match="view index"):
        instance_views(w, offsets, sizes, view_of + 1, view)
    with pytest.raises(ValueError, match="view index"):
        instance_views(w, offsets, sizes, view_of - 1, view)
    with pytest.raises(ValueError, match="one source size per view"):
        instance_views(w, offsets[:2], np.array([[40, 33], [33, 40]]), view_of[:2], view)
    with pytest.raises(ValueError, match="empty"):
        instance_views(w, offsets, sizes, view_of, [])
    with pytest.raises(ValueError, match="flat contiguous int32"):
        instance_views(w.float(), offsets, sizes, view_of, view)
    with pytest.raises(ValueError, match="bits"):
        instance_views(w, offsets, sizes, view_of, view, out="bool")
