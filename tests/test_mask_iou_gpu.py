"""csrc/mask_iou.hip on the device: the RLE decoder against the host definition, the pair counts against the dense
definition, the evaluator on the device against its CPU result, and the head's keep_bits planes.  Everything is
integer-exact: every comparison is equality."""
import copy
import math

import numpy as np
import pytest
import torch

from bm2f_amd import (VideoMaskFormerInference, YTVISEvaluator, YTVISGroundTruth, YTVISParams, evaluate_ytvis,
                      mask_pair_counts, pack_mask_bits, rle_encode, rle_to_bits, rle_to_bits_ragged, string_to_counts)
from bm2f_amd.mask_iou import pair_tiles
from ytvis_eval_cases import CONFIGS, FIELDS, flatten, load_fixture

pytestmark = pytest.mark.gpu

SIZES = [(h, w) for h in (1, 7, 33) for w in (1, 31, 32, 33, 64, 65)]
TA, TB, CHUNK = pair_tiles()


def _rand(shape, p, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < p


def _checker(h, w):
    return (torch.arange(h)[:, None] + torch.arange(w)[None]) % 2 == 1


def _single(h, w, *pixels):
    m = torch.zeros(h, w, dtype=torch.bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def _check_decode(masks, device, with_none=True):
    """masks (M, H, W) bool on the host: the device planes equal pack_mask_bits, and encode them back."""
    H, W = masks.shape[1:]
    rles = rle_encode(masks)
    given = rles[:1] + [None] + rles[1:] + [None] if with_none else rles
    zero = torch.zeros(1, H, W, dtype=torch.bool)
    want = pack_mask_bits(torch.cat([masks[:1], zero, masks[1:], zero]) if with_none else masks)
    got = rle_to_bits(given, device=device)
    assert got.device.type == "cuda" and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want)
    assert torch.equal(rle_to_bits(given), want)                      # the host definition
    back = rle_encode(got, width=W)                                   # the device encoder, from the decoded planes
    assert back == [r if r is not None else rle_encode(zero)[0] for r in given]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_sizes(size, device):
    H, W = size
    masks = torch.stack([_rand((H, W), 0.02, 1), _rand((H, W), 0.5, 2), _rand((H, W), 0.98, 3),
                         torch.zeros(H, W, dtype=torch.bool), torch.ones(H, W, dtype=torch.bool), _checker(H, W),
                         _single(H, W, (0, 0)), _single(H, W, (H - 1, W - 1))])
    _check_decode(masks, device)


def test_decode_run_edges(device):
    masks = torch.stack([
        _single(9, 40, (7, 31), (8, 31), (0, 32), (1, 32), (8, 5), (0, 6)),   # runs crossing a column boundary
        _single(9, 40, (8, 31), (8, 32), (8, 39), (8, 0)),                    # runs ending at a column end
        _single(9, 40, (0, 0)), _single(9, 40, (8, 39))])
    _check_decode(masks, device)


def test_decode_large_and_mixed_run_counts(device):
    one = _single(1056, 1000, (528, 500))
    _check_decode(one[None], device, with_none=False)
    mixed = torch.stack([torch.zeros(200, 300, dtype=torch.bool), _rand((200, 300), 0.5, 5), _single(200, 300, (7, 7)),
                         _checker(200, 300), torch.ones(200, 300, dtype=torch.bool), _rand((200, 300), 0.02, 6)])
    _check_decode(mixed, device)


def test_decode_uncompressed_and_all_none(device):
    m = _rand((3, 7, 33), 0.5, 9)
    rles = [dict(r, counts=string_to_counts(r["counts"])) for r in rle_encode(m)]
    assert torch.equal(rle_to_bits(rles, device=device).cpu(), pack_mask_bits(m))
    z = rle_to_bits([None, None], device=device, size=(7, 33))
    assert tuple(z.shape) == (2, 7, 2) and int(z.abs().sum()) == 0
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [7, 33], "counts": [5, 5]}], device=device)


def test_decode_uniform_equals_ragged(device):
    """The two decode kernels share one column decoder: the same eight masks (the 9 x 40 run edges, three 7 x 33 and a
    missing 7 x 33) through rle_to_bits, one size per call, and through one rle_to_bits_ragged call, word for word."""
    edges = [_single(9, 40, (7, 31), (8, 31), (0, 32), (1, 32), (8, 5), (0, 6)),
             _single(9, 40, (8, 31), (8, 32), (8, 39), (8, 0)), _single(9, 40, (0, 0)), _single(9, 40, (8, 39))]
    small = rle_encode(_rand((3, 7, 33), 0.5, 9))
    small.insert(1, None)
    rles = rle_encode(torch.stack(edges)) + small
    words, off, hw = rle_to_bits_ragged(rles, device=device, sizes=[None] * 5 + [(7, 33)] + [None] * 2)
    assert words.device.type == "cuda" and [tuple(s) for s in hw] == [(9, 40)] * 4 + [(7, 33)] * 4
    uniform = [*rle_to_bits(rles[:4], device=device), *rle_to_bits(rles[4:], device=device, size=(7, 33))]
    for m, plane in enumerate(uniform):
        assert torch.equal(words[off[m]:off[m] + plane.numel()], plane.reshape(-1)), m
    assert int(uniform[5].abs().sum()) == 0


def _dense(a, b):
    inter = (a[:, None] & b[None]).sum((2, 3, 4)).numpy()
    return inter, a.sum((2, 3)).numpy(), b.sum((2, 3)).numpy()


def _check_pairs(a, b, device):
    W = a.shape[-1]
    want = _dense(a, b)
    got = mask_pair_counts(pack_mask_bits(a).to(device), pack_mask_bits(b).to(device), W)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)
    return got


@pytest.mark.parametrize("da", [1, TA - 1, TA, TA + 1])
@pytest.mark.parametrize("db", [1, TB - 1, TB, TB + 1])
def test_pair_counts_tile_edges(da, db, device):
    """Every (Da, Db) around the instance tile, at T = 1 and 3, on sizes that cycle through SIZES."""
    n = (da * 7 + db) % len(SIZES)
    for T, (H, W) in ((1, SIZES[n]), (3, SIZES[(n + 5) % len(SIZES)]), (3, (33, 65))):
        _check_pairs(_rand((da, T, H, W), 0.5, da * 10 + db), _rand((db, T, H, W), 0.4, da * 10 + db + 100), device)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_counts_sizes(size, device):
    H, W = size
    for T in (1, 3):
        _check_pairs(_rand((2, T, H, W), 0.5, H + W + T), _rand((3, T, H, W), 0.5, H * W + T), device)


def test_pair_counts_several_chunks(device):
    """300 x 700: 6600 words per frame, more than one chunk and no multiple of it; 128-bit and 32-bit loads."""
    H, W, T = 300, 700, 2
    assert CHUNK < H * 22 < 2 * CHUNK
    a, b = _rand((2, T, H, W), 0.5, 1), _rand((2, T, H, W), 0.3, 2)
    want = _check_pairs(a, b, device)
    pa, pb = pack_mask_bits(a).to(device), pack_mask_bits(b).to(device)
    # tail bits set to ones in the input: unchanged counts
    tail = torch.zeros(22, dtype=torch.int32)
    tail[-1] = -(1 << (W % 32))
    dirty = mask_pair_counts(pa | tail.to(device), pb | tail.to(device), W)
    assert all(np.array_equal(x, y) for x, y in zip(dirty, want))
    # B as a strided view of a larger buffer (every second instance), and off the 16-byte grid (32-bit loads)
    big = torch.full((4, T, H, 22), -1, dtype=torch.int32, device=device)
    big[::2] = pb
    assert big[::2].data_ptr() == big.data_ptr() and not big[::2].is_contiguous()
    strided = mask_pair_counts(pa, big[::2], W)
    assert all(np.array_equal(x, y) for x, y in zip(strided, want))
    flat = torch.empty(pb.numel() + 1, dtype=torch.int32, device=device)
    shifted = flat[1:].view(pb.shape)
    shifted.copy_(pb)
    assert shifted.data_ptr() % 16 == 4
    narrow = mask_pair_counts(pa, shifted, W)
    assert all(np.array_equal(x, y) for x, y in zip(narrow, want))


def test_pair_counts_empty_side_and_identity(device):
    a = _rand((3, 2, 9, 70), 0.5, 4)
    pa = pack_mask_bits(a).to(device)
    inter, area_a, area_b = mask_pair_counts(pa[:0], pa, 70)
    assert inter.shape == (0, 3) and area_a.shape == (0, 2) and np.array_equal(area_b, a.sum((2, 3)).numpy())
    inter, area_a, area_b = mask_pair_counts(pa, pa, 70)              # identical A and B
    assert np.array_equal(np.diag(inter), area_a.sum(1)) and np.array_equal(area_a, area_b)


def test_pair_counts_repeatable_with_garbage_in_the_allocator(device):
    """Two runs, the freed blocks the workspace and output come from pre-filled with garbage: bitwise equal."""
    a, b = _rand((TA + 1, 2, 40, 100), 0.5, 7), _rand((TB + 1, 2, 40, 100), 0.5, 8)
    pa, pb = pack_mask_bits(a).to(device), pack_mask_bits(b).to(device)
    runs = []
    for fill in (0x5a5a5a5a, -1):
        junk = [torch.full((n,), fill, dtype=torch.int32, device=device) for n in (64, 1024, 16384, 1 << 20)]
        torch.cuda.synchronize()
        del junk                                                      # back to the caching allocator, not zeroed
        runs.append(mask_pair_counts(pa, pb, 100))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], _dense(a, b)))


# -------------------------------------------------------------------------------------------------------------------
# evaluator
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_ytvis_on_device_equals_cpu(name, device):
    gt, results, expected = load_fixture()
    p = YTVISParams()
    p.maxDets = list(CONFIGS[name])
    r = evaluate_ytvis(YTVISGroundTruth(gt), results, device=device, params=p)
    c = evaluate_ytvis(YTVISGroundTruth(gt), results, params=p)
    got = flatten(r.ious, r.evalImgs, r.precision, r.recall, r.scores, r.stats, 10)
    cpu = flatten(c.ious, c.evalImgs, c.precision, c.recall, c.scores, c.stats, 10)
    for f in FIELDS:
        assert np.array_equal(got[f], cpu[f]), f
        if f != "stats":
            assert np.array_equal(got[f], expected[name][f]), f


def _video_outputs(device, Q=12, K=3, T=2, h=20, w=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, Q, T, 3, 4, generator=g) * 3
    masks = torch.nn.functional.interpolate(low.flatten(0, 1), size=(h, w), mode="bilinear").view(1, Q, T, h, w)
    return {"pred_logits": (torch.randn(1, Q, K + 1, generator=g) * 2).to(device), "pred_masks": masks.to(device)}


def test_keep_bits_is_the_packed_output(device):
    head = VideoMaskFormerInference(3, test_topk_per_video=6)
    args = (_video_outputs(device), (80, 112), (75, 100), (90, 130))
    packed = head(*args, packed=True)
    for kw in ({}, {"packed": True}, {"rle": True}):
        r = head(*args, keep_bits=True, **kw)
        assert r["pred_bits"].device.type == "cuda" and r["pred_bits"].dtype == torch.int32
        assert torch.equal(r["pred_bits"].cpu(), torch.stack(packed["pred_masks"]))
        plain = head(*args, **kw)
        assert "pred_bits" not in plain and plain["pred_scores"] == r["pred_scores"]
        if kw.get("rle"):
            assert plain["pred_masks"] == r["pred_masks"]
        else:
            assert all(torch.equal(x, y) for x, y in zip(plain["pred_masks"], r["pred_masks"]))


def test_evaluator_from_kept_bits_equals_rle_route(device):
    head = VideoMaskFormerInference(3, test_topk_per_video=6)
    geometry = ((80, 112), (75, 100))
    id_map = {11: 0, 12: 1, 13: 2}
    videos, anns, outs = [], [], []
    for vid, seed in ((5, 0), (9, 1)):
        out = _video_outputs(device, seed=seed)
        plain = head(out, *geometry)
        videos.append({"id": vid, "height": 75, "width": 100, "length": 2})
        for rank, e in enumerate(np.argsort(plain["pred_scores"])[::-1][:3]):
            m = plain["pred_masks"][e]
            m = torch.roll(m, shifts=9, dims=-1) if rank == 1 else m
            anns.append({"id": len(anns) + 1, "video_id": vid, "category_id": plain["pred_labels"][e] + 11,
                         "iscrowd": 0, "segmentations": rle_encode(m), "areas": [int(f.sum()) for f in m]})
        outs.append((vid, out))
    gt = {"videos": videos, "annotations": anns, "categories": [{"id": 11 + i, "name": n} for i, n in enumerate("abc")]}
    metrics = []
    for kw in ({"rle": True}, {"rle": True, "keep_bits": True}, {"keep_bits": True}, {"packed": True, "keep_bits": True}):
        ev = YTVISEvaluator(copy.deepcopy(gt), id_map, class_names=list("abc"))
        for vid, out in outs:
            ev.process([{"video_id": vid, "length": 2}], head(out, *geometry, **kw))
        if "keep_bits" in kw:
            assert set(ev._counts) == {5, 9}                          # counted at process time, from the device planes
        metrics.append(ev.evaluate()["segm"])
    for m in metrics[1:]:
        assert m.keys() == metrics[0].keys()
        assert all(m[k] == metrics[0][k] or (math.isnan(m[k]) and math.isnan(metrics[0][k])) for k in m)
    assert metrics[0]["AP50"] > 0
