"""csrc/label_counts.hip on the device against the numpy path of bm2f_amd.label_counts (itself checked against
np.bincount in test_seg_eval_cpu.py), with the kernel's path forced to "lds", "global" and left on "auto".  Counts are
integers: every comparison is equality."""
import numpy as np
import pytest
import torch

from bm2f_amd import label_pair_counts, label_pair_counts_ragged
from bm2f_amd.label_counts import MAX_IDS, geometry

pytestmark = pytest.mark.gpu

PATHS = ["lds", "global", "auto"]
A_DTYPES = [torch.uint8, torch.int16, torch.int32]
B_DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64]


def _labels(n, hi, dtype, seed, runs=True):
    """n labels in [0, hi): piecewise constant runs of 4 to 11 pixels (as label maps are) or per-pixel random."""
    g = torch.Generator().manual_seed(seed)
    if not runs:
        return torch.randint(0, hi, (n,), generator=g).to(dtype)
    values = torch.randint(0, hi, (n // 4 + 1,), generator=g)
    return values.repeat_interleave(torch.randint(4, 12, values.shape, generator=g))[:n].contiguous().to(dtype)


def _pad_to(t, n):
    return torch.cat([t, t.new_zeros(n - t.numel())]) if t.numel() < n else t


def _pair(n, rows, cols, a_dtype, b_dtype, seed, runs=True):
    a = _pad_to(_labels(n, rows - 1, a_dtype, seed, runs), n)
    b = _pad_to(_labels(n, cols, b_dtype, seed + 1000, runs), n)
    return a, b


def _same(got, want):
    (gt, gb), (wt, wb) = got, want
    if isinstance(wt, list):
        assert len(gt) == len(wt) and all(np.array_equal(x, y) for x, y in zip(gt, wt))
    else:
        assert np.array_equal(gt, wt)
    assert np.array_equal(np.asarray(gb), np.asarray(wb))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pixels", [1, 63, 64, 65, 257, 300 * 300])
def test_pixel_counts(pixels, path, device):
    a, b = _pair(pixels, 6, 5, torch.uint8, torch.int16, pixels)
    a[0] = 255                                                        # the ignore label
    want = label_pair_counts(a, b, rows=6, cols=5, ignore=255)
    assert int(want[0].sum()) == pixels
    _same(label_pair_counts(a.to(device), b.to(device), rows=6, cols=5, ignore=255, path=path), want)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shared", [False, True])
def test_ragged_batch_at_odd_offsets(shared, path, device):
    """Five images cut out of one flat buffer per side at odd element offsets; one of them spans two chunks.  The
    buffers start on 16 bytes (asserted) and the batch's base is the lowest plane address rounded down to 16 bytes,
    so a is read with aligned loads whose head and tail vectors are masked (no a_off is a multiple of 8); b takes
    the aligned route where b_off - a_off is a multiple of 8 (images 1 and 2) and the scalar route elsewhere."""
    sizes = [1, 77, 64 * 8 + 3, 70001, 300]
    a_off = [1, 5, 91, 611, 70701]
    b_off = [3, 13, 99, 1000, 71111]                                  # b - a: 2, 8, 8, 389, 410
    rows, cols = 7, 9
    fa = torch.full((71200,), 99, dtype=torch.int16)
    fb = torch.full((71500,), -5, dtype=torch.int32)                   # whatever lies between the planes is never read as a label
    for k, (n, oa, ob) in enumerate(zip(sizes, a_off, b_off)):
        x, y = _pair(n, rows, cols, torch.int16, torch.int32, 10 + k)
        fa[oa:oa + n], fb[ob:ob + n] = x, y
    da, db = fa.to(device), fb.to(device)
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    assert all(o % 8 for o in a_off) and [(q - o) % 8 == 0 for o, q in zip(a_off, b_off)] == [False, True, True, False,
                                                                                               False]
    planes_a = [fa[o:o + n] for o, n in zip(a_off, sizes)]
    planes_b = [fb[o:o + n] for o, n in zip(b_off, sizes)]
    dev_a = [da[o:o + n] for o, n in zip(a_off, sizes)]
    dev_b = [db[o:o + n] for o, n in zip(b_off, sizes)]
    want = label_pair_counts_ragged(planes_a, planes_b, rows=rows, cols=cols, share_output=shared)
    assert not want[1].any()
    _same(label_pair_counts_ragged(dev_a, dev_b, rows=rows, cols=cols, share_output=shared, path=path), want)
    # host planes beside device planes: uploaded in one copy and counted in the same launch
    mixed_a = [p if k % 2 else d for k, (p, d) in enumerate(zip(planes_a, dev_a))]
    mixed_b = [d if k % 2 else p.numpy() for k, (p, d) in enumerate(zip(planes_b, dev_b))]
    _same(label_pair_counts_ragged(mixed_a, mixed_b, rows=rows, cols=cols, share_output=shared, path=path), want)


@pytest.mark.parametrize("path", ["lds", "global"])
@pytest.mark.parametrize("a_dtype", A_DTYPES, ids=str)
@pytest.mark.parametrize("b_dtype", B_DTYPES, ids=str)
def test_masked_heads_and_tails_on_an_aligned_base(a_dtype, b_dtype, path, device):
    """Every dtype pair with aligned loads of a whose first and last vectors hold a neighbour's elements: planes of
    1 to 70 pixels packed back to back at every residue of a_off mod 8 in a 16-byte aligned buffer, the neighbours'
    labels being valid labels (a wrong mask would count them).  b_off - a_off runs over 0, 8 and -16 (aligned loads
    of b, heads masked too) and 3, -5 and 9 (scalar loads of b beside aligned loads of a)."""
    rows, cols = 6, 7
    sizes = [1, 7, 3, 9, 15, 5, 17, 70, 6, 64, 8, 2]
    a_off, at = [], 1
    for n in sizes:
        a_off.append(at)
        at += n                                                       # back to back
    deltas = [0, 3, 8, -5, 0, 9, 8, -16, 3, 0, 8, -5]
    b_off = [o + 32 + d for o, d in zip(a_off, deltas)]
    assert {o % 8 for o in a_off} == {0, 1, 2, 4, 5, 6}
    fa = _labels(at + 64, rows - 1, a_dtype, 21, runs=False)          # valid labels everywhere, between the planes too
    fb = _labels(at + 128, cols, b_dtype, 22, runs=False)
    da, db = fa.to(device), fb.to(device)
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    host = ([fa[o:o + n] for o, n in zip(a_off, sizes)], [fb[o:o + n] for o, n in zip(b_off, sizes)])
    dev = ([da[o:o + n] for o, n in zip(a_off, sizes)], [db[o:o + n] for o, n in zip(b_off, sizes)])
    want = label_pair_counts_ragged(*host, rows=rows, cols=cols)
    assert [int(t.sum()) for t in want[0]] == sizes
    _same(label_pair_counts_ragged(*dev, rows=rows, cols=cols, path=path), want)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("table", [(2, 2), (151, 151), (258, 101)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_table_sizes(table, path, device):
    rows, cols = table
    lds_bins = geometry()[2]
    a, b = _pair(40000, rows, cols, torch.int16, torch.int16, rows)
    a2, b2 = _pair(5000, rows, cols, torch.int16, torch.int16, rows + 1, runs=False)
    want = label_pair_counts_ragged([a, a2], [b, b2], rows=rows, cols=cols)
    dev = ([a.to(device), a2.to(device)], [b.to(device), b2.to(device)])
    if path == "lds" and rows * cols > lds_bins:
        with pytest.raises(ValueError, match="LDS"):
            label_pair_counts_ragged(*dev, rows=rows, cols=cols, path=path)
        return
    _same(label_pair_counts_ragged(*dev, rows=rows, cols=cols, path=path), want)


def test_auto_crosses_the_lds_budget():
    lds_bins = geometry()[2]
    assert 151 * 151 <= lds_bins < 258 * 101


@pytest.mark.parametrize("path", ["lds", "global"])
@pytest.mark.parametrize("a_dtype", A_DTYPES, ids=str)
@pytest.mark.parametrize("b_dtype", B_DTYPES, ids=str)
def test_dtypes(a_dtype, b_dtype, path, device):
    a, b = _pair(3001, 9, 11, a_dtype, b_dtype, 5)
    a[7:19] = 100                                                     # ignore
    a[40] = 50                                                        # bad in a
    b[41] = 11                                                        # bad in b
    if b_dtype == torch.int64:
        b[42], b[43] = 2 ** 40, -2 ** 40                              # no int32 column
    if b_dtype != torch.uint8:
        b[44] = -1
    want = label_pair_counts(a, b, rows=9, cols=11, ignore=100)
    assert want[1] >= 2
    _same(label_pair_counts(a.to(device), b.to(device), rows=9, cols=11, ignore=100, path=path), want)


@pytest.mark.parametrize("path", PATHS)
def test_wave_aggregation_extremes(path, device):
    # one bin for 90,000 pixels: every wave merges its 64 lanes into one add
    a = torch.full((300, 300), 3, dtype=torch.uint8)
    b = torch.full((300, 300), 2, dtype=torch.int16)
    table, bad = label_pair_counts(a.to(device), b.to(device), rows=5, cols=4, path=path)
    assert table[3, 2] == 90000 and table.sum() == 90000 and bad == 0
    # the 64 lanes of a wave hold 64 different keys at every step: lane l of every wave reads pixels 8 l .. 8 l + 7
    lane = (torch.arange(4096) // 8) % 64
    a = (lane // 8).to(torch.uint8)
    b = (lane % 8).to(torch.int16)
    want = label_pair_counts(a, b, rows=9, cols=8)
    assert (want[0][:8] == 64).all()
    _same(label_pair_counts(a.to(device), b.to(device), rows=9, cols=8, path=path), want)


@pytest.mark.parametrize("path", PATHS)
def test_id_list_mode(path, device):
    big = 2 ** 24 - 1
    ids = [0, 1, big]
    a = torch.tensor([0, 1, big, 5, big, big, 1, 7, 0, 2 ** 24], dtype=torch.int32).repeat(37)    # 5, 7, 2^24: "other"
    b = _pad_to(_labels(a.numel(), 6, torch.int32, 3), a.numel())
    b[5] = 6                                                          # bad in b
    want = label_pair_counts(a, b, rows=4, cols=6, ids=ids)
    assert want[0][3].sum() > 0 and want[1] == 1
    _same(label_pair_counts(a.to(device), b.to(device), rows=4, cols=6, ids=ids, path=path), want)
    # the longest list, with different lists per image
    g = torch.Generator().manual_seed(4)
    many = torch.sort(torch.randperm(5000, generator=g)[:MAX_IDS]).values
    few = many[::7][:100]
    a1 = torch.randint(0, 5000, (20000,), generator=g).to(torch.int32)
    a2 = _pad_to(_labels(9000, 5000, torch.int32, 6), 9000)
    b1 = _pad_to(_labels(20000, 3, torch.uint8, 7), 20000)
    b2 = _pad_to(_labels(9000, 3, torch.uint8, 8), 9000)
    kw = dict(rows=[MAX_IDS + 1, 101], cols=[3, 3], ids=[many.tolist(), few.tolist()])
    want = label_pair_counts_ragged([a1, a2], [b1, b2], **kw)
    _same(label_pair_counts_ragged([a1.to(device), a2.to(device)], [b1.to(device), b2.to(device)], path=path, **kw),
          want)


def test_empty_inputs(device):
    tables, bad = label_pair_counts_ragged([], [], rows=3, cols=3)
    assert tables == [] and bad.size == 0
    z = torch.zeros(0, dtype=torch.uint8, device=device)
    a, b = _pair(100, 3, 3, torch.uint8, torch.uint8, 1)
    for path in PATHS:
        table, bad = label_pair_counts(z, z, rows=3, cols=3, path=path)
        assert table.shape == (3, 3) and not table.any() and bad == 0
        _same(label_pair_counts_ragged([z, a.to(device), z], [z, b.to(device), z], rows=3, cols=3, path=path),
              label_pair_counts_ragged([z.cpu(), a, z.cpu()], [z.cpu(), b, z.cpu()], rows=3, cols=3))


@pytest.mark.parametrize("path", ["lds", "global"])
def test_repeatable(path, device):
    a, b = _pair(200000, 20, 20, torch.uint8, torch.int16, 9, runs=False)
    da, db = a.to(device), b.to(device)
    first = label_pair_counts(da, db, rows=20, cols=20, path=path)
    second = label_pair_counts(da, db, rows=20, cols=20, path=path)
    _same(first, second)
    _same(first, label_pair_counts(a, b, rows=20, cols=20))
