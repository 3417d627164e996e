"""``m2f_bits_views`` (csrc/bits_views.hip) on the device against Pillow's recorded outputs
(tests/golden/instance_views.npz) and against the CPU definition, bit for bit, in both output forms, on the cases of
tests/instance_view_cases.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import instance_view_cases as ivc
from bm2f_amd import _native
from bm2f_amd.image_views import View
from bm2f_amd.instance_views import bit_boxes_ragged, instance_views

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_views.npz")
SENTINEL = {"bits": -1, "uint8": 0xA5}


def run_case(case, out, device, garbage=None, **kw):
    words, offsets, sizes, view_of = ivc.ragged([ivc.case_masks(case["hw"])], garbage)
    return instance_views(torch.from_numpy(words).to(device), offsets, sizes, view_of, [case["view"]], out=out, **kw)


def same(got, want):
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w)
    assert got[3] == want[3]


@pytest.mark.parametrize("out", ["bits", "uint8"])
@pytest.mark.parametrize("case", ivc.CASES, ids=lambda c: c["name"])
def test_case_equals_the_fixture_and_the_cpu_definition(case, out, device):
    """Garbage tail bits and padding words in the source, a sentinel in the output: every word of every plane is
    overwritten, tail bits are zero, and the result is the one of the clean source."""
    want = run_case(case, out, "cpu")
    Hc, Wc = ivc.canvas_of(case["view"])
    shape = (6, Hc, (Wc + 31) // 32) if out == "bits" else (6, Hc, Wc)
    into = torch.full(shape, SENTINEL[out], dtype=want[0].dtype, device=device)
    got = run_case(case, out, device, garbage=np.random.default_rng(7), into=into)
    assert got[0] is into
    same(got, want)
    dense = got[0].cpu().numpy()
    if out == "bits":
        dense, clean = ivc.unpack(dense, Wc)
        assert clean, "a tail bit is set"
    assert np.array_equal(dense, ivc.golden_masks(np.load(GOLDEN), case["name"], (Hc, Wc)))


@pytest.mark.parametrize("out", ["bits", "uint8"])
def test_batch_with_0_1_and_70_instances(out, device):
    """One call for four images of different sizes and instance counts, padded to a multiple of 32; twice, for
    bitwise repeatability of masks and stats."""
    cases, lists = ivc.batch_masks()
    words, offsets, sizes, view_of = ivc.ragged(lists, np.random.default_rng(9))
    views = [c["view"] for c in cases]
    want = instance_views(torch.from_numpy(words), offsets, sizes, view_of, views, size_divisibility=32, out=out)
    w = torch.from_numpy(words).to(device)
    got = instance_views(w, offsets, sizes, view_of, views, size_divisibility=32, out=out)
    again = instance_views(w, offsets, sizes, view_of, views, size_divisibility=32, out=out)
    same(got, want)
    for a, b in zip(got[:3], again[:3]):
        assert torch.equal(a, b)
    wb, wa = ivc.bitmask_boxes(want[0].numpy() if out == "uint8" else ivc.unpack(want[0].numpy(), 96)[0])
    assert np.array_equal(got[1].cpu().numpy(), wb) and np.array_equal(got[2].cpu().numpy(), wa)


def test_bit_boxes_ragged(device):
    a, b = ivc.case_masks((40, 33)), ivc.case_masks((17, 70))
    words, offsets, sizes, _ = ivc.ragged([a, b], np.random.default_rng(2))
    want = bit_boxes_ragged(torch.from_numpy(words), offsets, sizes)
    got = bit_boxes_ragged(torch.from_numpy(words).to(device), offsets, sizes)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)


def test_bad_tables_raise_before_any_launch(device):
    """The Python checks, then the entry point's own checks of the host tables (reached by calling it directly):
    the output keeps its sentinel, so nothing was launched."""
    masks = ivc.case_masks((40, 33))
    words, offsets, sizes, view_of = ivc.ragged([masks])
    w, view = torch.from_numpy(words).to(device), [View(size=(20, 20))]
    with pytest.raises(ValueError, match="does not fit"):
        instance_views(w, offsets + words.size, sizes, view_of, view)
    with pytest.raises(ValueError, match="positive"):
        instance_views(w, offsets, sizes * np.array([[1, 0]]), view_of, view)
    with pytest.raises(ValueError, match="view index"):
        instance_views(w, offsets, sizes, view_of + 1, view)

    mod = __import__("bm2f_amd.instance_views", fromlist=["_plan"])
    good = mod._mask_table(w, offsets, sizes, view_of, view)
    plan = mod._plan(view, good)
    dev = torch.from_numpy(np.concatenate((plan.rows.reshape(-1).view(np.int32), good.reshape(-1).view(np.int32),
                                           plan.tables))).to(device)
    out = torch.full((6, 20, 1), -1, dtype=torch.int32, device=device)
    stats = torch.full((6, 5), -1, dtype=torch.int32, device=device)
    ws = torch.empty(6 * 5, dtype=torch.int32, device=device)

    def call(table, rows=plan.rows):
        table = np.ascontiguousarray(table, dtype=np.int64)
        _native.call("m2f_bits_views", w.data_ptr(), w.numel(), rows.ctypes.data_as(ctypes.c_void_p), dev.data_ptr(), 1,
                     dev.data_ptr() + (20 + 6 * 4) * 8, plan.tables.size, table.ctypes.data_as(ctypes.c_void_p),
                     dev.data_ptr() + 20 * 8, 6, 0, out.data_ptr(), 20, 20, stats.data_ptr(), ws.data_ptr(), ws.numel(),
                     _native.stream(device))

    for col, value in ((0, words.size), (0, -1), (1, 0), (2, -3), (2, 34), (3, 1), (3, -1)):
        bad = good.copy()
        bad[4, col] = value
        with pytest.raises(_native.NativeError, match="mask 4"):
            call(bad)
    rows = plan.rows.copy()
    rows[0, 15] = plan.tables.size                           # the y table leaves the tables
    with pytest.raises(_native.NativeError, match="view 0"):
        call(good, rows)
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((stats == -1).all())
    call(good)                                               # and the good tables pass
    torch.cuda.synchronize()
    want = instance_views(torch.from_numpy(words), offsets, sizes, view_of, view)
    assert torch.equal(out.cpu(), want[0]) and torch.equal(stats[:, 4].cpu(), want[2])
