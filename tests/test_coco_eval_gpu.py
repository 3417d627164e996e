"""The ragged kernels of csrc/mask_iou.hip on the device: the decoder against the CPU definition, the pair counts
against the numpy restatement and against the single-size kernel, and evaluate_coco on the device against its CPU
result.  Everything is integer-exact: every comparison is equality."""
import copy

import numpy as np
import pytest
import torch

from bm2f_amd import (COCOGroundTruth, COCOParams, evaluate_coco, mask_pair_counts, mask_pair_counts_ragged,
                      pack_mask_bits, rle_encode, rle_to_bits_ragged)
from bm2f_amd.mask_iou import pair_tiles
from coco_eval_cases import CONFIGS, FIELDS, flatten, load_fixture

pytestmark = pytest.mark.gpu

TA, TB, CHUNK = pair_tiles()
DECODE_SIZES = [(1, 1), (2, 31), (7, 32), (3, 33), (5, 64), (4, 65), (70, 2100), (9, 127)]


def _rand(shape, p, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < p


def test_decode_ragged_equals_cpu(device):
    masks = [_rand(s, 0.4, i) for i, s in enumerate(DECODE_SIZES)]
    masks[2] = torch.zeros(7, 32, dtype=torch.bool)
    masks[3] = torch.ones(3, 33, dtype=torch.bool)
    rles = [rle_encode(m[None])[0] for m in masks]
    rles.insert(5, None)
    sizes = [None] * 5 + [(6, 70)] + [None] * 3
    got, off, hw = rle_to_bits_ragged(rles, device=device, sizes=sizes)
    want, off_c, hw_c = rle_to_bits_ragged(rles, sizes=sizes)
    assert got.device.type == "cuda" and got.dtype == torch.int32 and got.shape == want.shape
    assert np.array_equal(off, off_c) and np.array_equal(hw, hw_c)
    host = got.cpu()
    dense = masks[:5] + [torch.zeros(6, 70, dtype=torch.bool)] + masks[5:]
    for m, (H, W) in enumerate(hw):
        n = H * ((W + 31) // 32)
        plane = host[off[m]:off[m] + n]
        assert torch.equal(plane, want[off[m]:off[m] + n]), m            # word for word, tail bits included
        assert torch.equal(plane.view(H, -1), pack_mask_bits(dense[m][None])[0]), m
        if W % 32:
            assert int((plane.view(H, -1)[:, -1] >> (W % 32)).abs().sum()) == 0


# (H, W, na, nb): widths 1, 31, 32, 33, 65 and 127, word counts off the multiples of 4, a plane longer than a chunk,
# na and nb around the tiles, and groups with an empty side
def _group_shapes():
    return [(3, 1, 1, 1), (5, 31, TA, TB), (7, 32, TA + 1, TB + 1), (3, 33, 2 * TA + 1, 2 * TB + 1), (9, 65, 1, TB),
            (9, 127, TA, 1), (70, 2100, 2, TB + 1), (5, 33, 0, 3), (5, 65, 2, 0), (4, 4, 0, 0), (6, 100, 3, 2)]


def _build(shapes, device, aligned, seed=0):
    """-> (words on the device, groups, dense masks per group); ``aligned`` pads planes to 4 words, otherwise the
    planes are packed back to back behind one word, off the 16-byte grid.  Tail bits are set in the input."""
    planes, groups, dense, at = [], [], [], 0 if aligned else 1
    if not aligned:
        planes.append(torch.full((1,), -1, dtype=torch.int32))
    for g, (H, W, na, nb) in enumerate(shapes):
        a, b = _rand((na, H, W), 0.5, seed + 2 * g), _rand((nb, H, W), 0.4, seed + 2 * g + 1)
        offs = []
        for m in torch.cat([a, b]):
            p = pack_mask_bits(m[None])[0]
            if W % 32:
                p[:, -1] |= -(1 << (W % 32))                          # tail bits the kernel must ignore
            p = p.reshape(-1)
            offs.append(at)
            planes.append(p)
            at += p.numel()
            pad = (-at) % 4 if aligned else 0
            planes.append(torch.full((pad,), -1, dtype=torch.int32))  # padding words hold ones too
            at += pad
        groups.append((H, W, offs[:na], offs[na:]))
        dense.append((a, b))
    return torch.cat(planes).to(device), groups, dense


def _same(x, y):
    return len(x) == len(y) and all(p.dtype == np.int64 and p.shape == q.shape and np.array_equal(p, q)
                                    for gx, gy in zip(x, y) for p, q in zip(gx, gy))


@pytest.mark.parametrize("aligned", [True, False], ids=["padded", "packed"])
def test_pair_counts_ragged(aligned, device):
    shapes = _group_shapes()
    assert CHUNK < 70 * 66 < 2 * CHUNK and (70 * 66) % 4 == 0 and (3 * 2) % 4 and (9 * 3) % 4
    words, groups, dense = _build(shapes, device, aligned)
    if not aligned:
        assert any(o % 4 for g in groups for o in g[2] + g[3])
    got = mask_pair_counts_ragged(words, groups)
    assert _same(got, mask_pair_counts_ragged(words.cpu(), groups))    # the numpy restatement
    for (H, W, na, nb), (inter, area_a, area_b), (a, b) in zip(shapes, got, dense):
        assert inter.shape == (na, nb) and area_a.shape == (na,) and area_b.shape == (nb,)
        assert np.array_equal(inter, (a[:, None] & b[None]).sum((2, 3)).numpy())
        assert np.array_equal(area_a, a.sum((1, 2)).numpy()) and np.array_equal(area_b, b.sum((1, 2)).numpy())
        # the single-size kernel, group by group with T = 1
        one = mask_pair_counts(pack_mask_bits(a[:, None]).to(device), pack_mask_bits(b[:, None]).to(device), W)
        assert np.array_equal(one[0], inter)
        assert np.array_equal(one[1].reshape(-1), area_a) and np.array_equal(one[2].reshape(-1), area_b)
    # bitwise repeatable, with garbage in the blocks the workspace and the output come from
    junk = [torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device=device) for n in (64, 1024, 16384, 1 << 20)]
    torch.cuda.synchronize()
    del junk
    assert _same(mask_pair_counts_ragged(words, groups), got)
    # one group alone and inside the batch agree
    for g in (3, 6, 7):
        alone = mask_pair_counts_ragged(words, [groups[g]])
        assert _same(alone, [got[g]])


def test_pair_counts_ragged_last_plane_without_padding(device):
    """Aligned planes whose word count is no multiple of 4, the last one ending the buffer: a four-word read of it
    would leave the buffer, so its workgroup must take the 32-bit path (and the others may stay wide)."""
    shapes = [(70, 2100, 1, 1), (3, 33, 2, 1), (9, 65, 1, 2)]
    words, groups, dense = _build(shapes, device, aligned=True)
    last = groups[-1][3][-1]
    assert (9 * 3) % 4 and last % 4 == 0 and words.numel() > last + 27
    words = words[:last + 27].clone()                                 # nothing behind the last plane
    assert words.numel() % 4 and words.data_ptr() % 16 == 0
    got = mask_pair_counts_ragged(words, groups)
    assert _same(got, mask_pair_counts_ragged(words.cpu(), groups))
    for (inter, area_a, area_b), (a, b) in zip(got, dense):
        assert np.array_equal(inter, (a[:, None] & b[None]).sum((2, 3)).numpy())
        assert np.array_equal(area_a, a.sum((1, 2)).numpy()) and np.array_equal(area_b, b.sum((1, 2)).numpy())


def test_rle_pair_counts_ragged_on_device_equals_cpu(device):
    from bm2f_amd.mask_iou import rle_pair_counts_ragged
    masks = [_rand(s, 0.4, i) for i, s in enumerate(DECODE_SIZES)]
    rles = [rle_encode(m[None])[0] for m in masks] + [None]
    sizes = [None] * len(masks) + [(9, 127)]
    groups = [(70, 2100, [6, 6], [6]), (9, 127, [7, 8], [8, 7]), (3, 33, [], [3]), (1, 1, [], []), (4, 65, [5], [])]
    got = rle_pair_counts_ragged(rles, groups, device=device, sizes=sizes)
    assert _same(got, rle_pair_counts_ragged(rles, groups, sizes=sizes))
    assert got[0][1].tolist() == [int(masks[6].sum())] * 2 and got[1][0][0, 1] == int(masks[7].sum())


def _flat(r):
    return flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, 10)


@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c[1] == "segm"])
def test_evaluate_coco_on_device_equals_cpu(name, device):
    gt, results, expected = load_fixture()
    max_dets, _ = CONFIGS[name]
    p = COCOParams()
    p.maxDets = list(max_dets)
    cpu = _flat(evaluate_coco(COCOGroundTruth(copy.deepcopy(gt)), results, params=p))
    # the default batch, several batches, and one image per batch
    for kw in ({}, {"batch_bytes": 300_000}, {"batch_bytes": 1}):
        got = _flat(evaluate_coco(COCOGroundTruth(copy.deepcopy(gt)), results, device=device, params=p, **kw))
        for f in FIELDS:
            assert np.array_equal(got[f], cpu[f]), (f, kw)
            assert np.array_equal(got[f], expected[name][f]), (f, kw)
