"""COCO RLE on the host (no GPU): the definition of bm2f_amd.rle against a per-pixel loop written here, the hand
vectors, the heads' rle options on CPU tensors, the result writers and the C entry points' argument checks.

The hand vectors were derived by hand from the format as bm2f_amd/rle.py states it and checked with the loop below;
they were NOT checked against a pycocotools run (pycocotools is not a dependency; the last test compares against it
where it happens to be installed)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from bm2f_amd import (MaskFormerInference, VideoMaskFormerInference, _native, counts_to_string,
                      instances_to_coco_json, instances_to_coco_json_video, pack_mask_bits, rle_area, rle_decode,
                      rle_encode, string_to_counts)
from bm2f_amd.rle import _char_bound


def loop_counts(mask):
    """Run lengths of a (H, W) mask read column-major, starting with a run of zeros."""
    H, W = mask.shape
    counts, prev, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            v = int(mask[y, x])
            if v != prev:
                counts.append(run)
                run, prev = 0, v
            run += 1
    counts.append(run)
    return counts


def loop_string(counts):
    s = ""
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            if more:
                c |= 0x20
            s += chr(c + 48)
    return s


def _box():
    m = torch.zeros(5, 7, dtype=torch.bool)
    m[1:4, 2:5] = True
    return m


def _checker(h, w):
    return (torch.arange(h)[:, None] + torch.arange(w)[None]) % 2 == 1


HAND = [
    (torch.zeros(4, 4, dtype=torch.bool), [16], "`0"),
    (torch.ones(4, 4, dtype=torch.bool), [0, 16], "0`0"),
    (_box(), [11, 3, 2, 3, 2, 3, 11], ";320009"),
    (_checker(6, 6), None, "1110010O0010O0010O0010O0010O000"),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_vectors(case):
    mask, counts, string = HAND[case]
    for r in (rle_encode(mask)[0], rle_encode(pack_mask_bits(mask), width=mask.shape[1])[0]):
        assert r == {"size": list(mask.shape), "counts": string}
        got = string_to_counts(r["counts"])
        if counts is None:
            assert len(got) == 31 and got == loop_counts(mask)
        else:
            assert got == counts
            assert counts_to_string(counts) == string


@pytest.mark.parametrize("size", [(1, 1), (5, 7), (33, 65), (64, 31)])
@pytest.mark.parametrize("p", [0.5, 0.02, 0.98])
def test_host_encode_equals_loop(size, p):
    H, W = size
    g = torch.Generator().manual_seed(H * 1000 + W + int(p * 100))
    masks = torch.rand(3, H, W, generator=g) < p
    from_bool = rle_encode(masks)
    from_bits = rle_encode(pack_mask_bits(masks), width=W)
    from_u8 = rle_encode(masks.to(torch.uint8) * 255)
    for i in range(3):
        counts = loop_counts(masks[i])
        want = {"size": [H, W], "counts": loop_string(counts)}
        assert from_bool[i] == want and from_bits[i] == want and from_u8[i] == want
        assert string_to_counts(want["counts"]) == counts
        assert torch.equal(rle_decode(want), masks[i])
        assert rle_area(want) == int(masks[i].sum())
        assert len(want["counts"]) <= _char_bound(len(counts), H * W)


def test_leading_dimensions_flatten():
    g = torch.Generator().manual_seed(3)
    masks = torch.rand(2, 3, 9, 11, generator=g) < 0.4
    assert rle_encode(masks) == [r for q in masks for r in rle_encode(q)]
    assert rle_encode(masks[0, 0]) == rle_encode(masks[:1, :1])
    assert rle_encode(masks[:0]) == []
    with pytest.raises(ValueError):
        rle_encode(masks.float())
    with pytest.raises(ValueError):
        rle_encode(pack_mask_bits(masks), width=40)


def test_string_roundtrip():
    for counts in ([5, 100, 3, 2, 1, 7],                              # counts[i] < counts[i - 2]: negative deltas
                   [15, 16, 31, 32, 2 ** 15, 2 ** 20],
                   [2 ** 20, 1, 2 ** 15, 32, 31, 16, 15, 1, 0 + 1],
                   [0, 2 ** 31 - 1], [0], [16], [2 ** 20]):
        s = counts_to_string(counts)
        assert s == loop_string(counts)
        assert string_to_counts(s) == counts
        assert string_to_counts(s.encode("ascii")) == counts
    assert len(counts_to_string([2 ** 31 - 1])) == 7
    assert len(counts_to_string([2 ** 20])) == 5


def test_char_bound_holds_for_dense_and_sparse_masks():
    """The device path sizes its copy by _char_bound from (number of counts, pixels) alone."""
    g = torch.Generator().manual_seed(11)
    masks = [_checker(40, 37), torch.zeros(1056, 1000, dtype=torch.bool), torch.rand(64, 64, generator=g) < 0.5]
    one = torch.zeros(1056, 1000, dtype=torch.bool)
    one[528, 500] = True
    stripes = torch.zeros(600, 40, dtype=torch.bool)
    stripes[::2] = True                                               # alternating long and short counts
    stripes[:, ::3] = True
    for m in masks + [one, stripes]:
        r = rle_encode(m)[0]
        n = len(string_to_counts(r["counts"]))
        assert len(r["counts"]) <= _char_bound(n, m.numel())


def _video_outputs(Q=12, K=5, T=3, h=20, w=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"pred_logits": torch.randn(1, Q, K + 1, generator=g) * 2,
            "pred_masks": torch.randn(1, Q, T, h, w, generator=g) * 3}


def test_video_head_rle_on_cpu():
    out = _video_outputs()
    head = VideoMaskFormerInference(5)
    args = (out, (80, 112), (75, 100), (90, 130))
    plain, enc = head(*args), head(*args, rle=True)
    assert enc["rle"] is True and "rle" not in plain
    assert enc["pred_scores"] == plain["pred_scores"] and enc["pred_labels"] == plain["pred_labels"]
    assert len(enc["pred_masks"]) == len(plain["pred_masks"]) == 10
    for e, m in zip(enc["pred_masks"], plain["pred_masks"]):
        assert e == rle_encode(m) and len(e) == 3
        assert e[0]["size"] == [90, 130]
    with pytest.raises(ValueError):
        head(*args, packed=True, rle=True)


def _image_outputs(B=2, Q=12, K=5, h=16, w=24, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"pred_logits": torch.randn(B, Q, K + 1, generator=g) * 2,
            "pred_masks": torch.randn(B, Q, h, w, generator=g) * 3}


def test_image_head_instance_rle_on_cpu():
    out = _image_outputs()
    head = MaskFormerInference(num_classes=5, semantic_on=False, instance_on=True, test_topk_per_image=7)
    args = (out, (64, 96), [(60, 90), (64, 70)], [(45, 67), (64, 70)])
    plain, enc = head(*args), head(*args, instance_rle=True)
    for b, size in enumerate([(45, 67), (64, 70)]):
        p, e = plain[b]["instances"], enc[b]["instances"]
        assert "pred_masks" not in e and "pred_masks_rle" not in p
        assert e["pred_masks_rle"] == rle_encode(p["pred_masks"] > 0)
        assert len(e["pred_masks_rle"]) == 7 and e["pred_masks_rle"][0]["size"] == list(size)
        assert e["image_size"] == size
        for k in ("scores", "pred_classes", "pred_boxes"):
            assert torch.equal(e[k], p[k])


def test_writers_return_json():
    out = _video_outputs()
    head = VideoMaskFormerInference(5)
    args = (out, (80, 112), (75, 100))
    inputs = [{"video_id": 17, "length": 3}]
    want = None
    for kw in ({}, {"packed": True}, {"rle": True}):
        res = instances_to_coco_json_video(inputs, head(*args, **kw))
        assert len(res) == 10
        for r in res:
            assert set(r) == {"video_id", "score", "category_id", "segmentations"}
            assert r["video_id"] == 17 and len(r["segmentations"]) == 3
            assert all(isinstance(s["counts"], str) and s["size"] == [75, 100] for s in r["segmentations"])
        assert json.loads(json.dumps(res)) == res
        want = want or res
        assert res == want
    with pytest.raises(AssertionError):
        instances_to_coco_json_video(inputs * 2, head(*args))

    img = MaskFormerInference(num_classes=5, semantic_on=False, instance_on=True, test_topk_per_image=7)
    iargs = (_image_outputs(), (64, 96), [(60, 90), (64, 70)])
    for kw in ({}, {"instance_rle": True}):
        ins = img(*iargs, **kw)[1]["instances"]
        ins["pred_boxes"] = torch.tensor([[1.0, 2.0, 11.0, 22.0]]).repeat(7, 1)
        res = instances_to_coco_json(ins, 42)
        assert len(res) == 7
        for r in res:
            assert set(r) == {"image_id", "category_id", "bbox", "score", "segmentation"}
            assert r["image_id"] == 42 and r["bbox"] == [1.0, 2.0, 10.0, 20.0]
            assert isinstance(r["segmentation"]["counts"], str) and r["segmentation"]["size"] == [64, 70]
        assert json.loads(json.dumps(res)) == res
    assert instances_to_coco_json({"scores": torch.zeros(0), "pred_classes": torch.zeros(0), "pred_boxes":
                                   torch.zeros(0, 4), "pred_masks": torch.zeros(0, 4, 4)}, 1) == []


def test_c_entry_argument_checks():
    """Null pointers, H * W >= 2^31, short strides and bad sizes are refused before any HIP call: the fake
    pointers never reach a kernel."""
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    L = ctypes.c_int64
    rc = lib.m2f_rle_col_counts(None, 1, None, 1, 1, 4, 4, L(4), L(16), p, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 1, 1, 4, 4, L(4), L(16), None, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_positions(p, 1, None, 1, 1, 4, 4, L(4), L(16), None, p, L(8), None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_deltas(p, None, 1, 4, L(8), p, p, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_chars(p, p, p, L(8), None, L(8), None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    for form in (0, 1):
        rc = lib.m2f_rle_col_counts(p, form, None, 1, 1, 1 << 16, 1 << 15, L(1 << 15), L(1 << 31), p, None)
        assert rc == 1 and b"32-bit" in lib.m2f_last_error()
        rc = lib.m2f_rle_positions(p, form, None, 1, 1, 1 << 16, 1 << 15, L(1 << 15), L(1 << 31), p, p, L(8), None)
        assert rc == 1 and b"32-bit" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 1, 1, 4, 40, L(39), L(160), p, None)
    assert rc == 1 and b"row stride" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 0, None, 1, 1, 4, 40, L(1), L(8), p, None)       # 40 bits need two words
    assert rc == 1 and b"row stride" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 2, 2, 4, 40, L(40), L(100), p, None)
    assert rc == 1 and b"plane stride" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 1, 0, 4, 4, L(4), L(16), p, None)
    assert rc == 1 and b"positive" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 2, None, 1, 1, 4, 4, L(4), L(16), p, None)
    assert rc == 1 and b"form" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 1, 2, 4, 4, L(4), L(16), p, None)       # two masks, one source plane
    assert rc == 1 and b"source planes" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(ctypes.c_void_p((1 << 20) + 1), 0, None, 1, 1, 4, 4, L(1), L(4), p, None)
    assert rc == 1 and b"aligned" in lib.m2f_last_error()
    rc = lib.m2f_rle_col_counts(p, 1, None, 70000, 70000, 4, 4, L(4), L(16), p, None)
    assert rc == 3
    rc = lib.m2f_rle_deltas(p, p, 4, 4, L(3), p, p, None)                            # fewer counts than masks
    assert rc == 1
    rc = lib.m2f_rle_chars(p, p, p, L(0), p, L(8), None)
    assert rc == 1
    _native.get_option("infer_video_cap")                                            # a success clears the message
    assert lib.m2f_last_error() == b""


def test_against_pycocotools_where_installed():
    mask_util = pytest.importorskip("pycocotools.mask")
    g = torch.Generator().manual_seed(5)
    for size, p in (((33, 65), 0.5), ((64, 31), 0.02), ((5, 7), 0.98), ((200, 300), 0.5)):
        m = torch.rand(*size, generator=g) < p
        want = mask_util.encode(np.asfortranarray(m.numpy().astype(np.uint8)))
        assert rle_encode(m)[0] == {"size": list(want["size"]), "counts": want["counts"].decode("ascii")}
