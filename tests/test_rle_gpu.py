"""COCO RLE on the device: the kernels of csrc/rle.hip against the host definition, byte for byte, in both input
forms, and the two heads' rle options against their own unencoded results.  Encoding is integer-exact: every
comparison is equality."""
import pytest
import torch

from bm2f_amd import MaskFormerInference, VideoMaskFormerInference, pack_mask_bits, rle_encode

pytestmark = pytest.mark.gpu


def _rand(shape, p, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < p


def _checker(h, w):
    return (torch.arange(h)[:, None] + torch.arange(w)[None]) % 2 == 1


def _single(h, w, *pixels):
    m = torch.zeros(h, w, dtype=torch.bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def _cases():
    c = {"1x1_zero": torch.zeros(1, 1, dtype=torch.bool), "1x1_one": torch.ones(1, 1, dtype=torch.bool),
         "1x33": _rand((1, 33), 0.5, 1), "33x1": _rand((33, 1), 0.5, 2)}
    for i, (h, w) in enumerate([(7, 32), (7, 33), (7, 64), (9, 65)]):
        for p in (0.5, 0.02, 0.98):
            c[f"{h}x{w}_p{p}"] = _rand((h, w), p, 10 * i + int(p * 100))
    c["33x65_zero"] = torch.zeros(33, 65, dtype=torch.bool)
    c["33x65_one"] = torch.ones(33, 65, dtype=torch.bool)
    c["33x65_checker"] = _checker(33, 65)
    c["pixel0"] = _single(9, 40, (0, 0))
    # a set run from the last row of column x into the first row of column x + 1: no transition there
    c["run_crosses_columns"] = _single(9, 40, (7, 31), (8, 31), (0, 32), (1, 32), (8, 5), (0, 6))
    # the reverse: last row set, next column's first row clear
    c["run_ends_at_column_end"] = _single(9, 40, (8, 31), (8, 32), (8, 39), (8, 0))
    c["3x700"] = _rand((3, 700), 0.5, 7)
    c["1056x1000_zero"] = torch.zeros(1056, 1000, dtype=torch.bool)
    c["1056x1000_centre"] = _single(1056, 1000, (528, 500))
    return c


CASES = _cases()


def _device_both_forms(mask, device):
    W = mask.shape[-1]
    d = mask.to(device)
    return rle_encode(d), rle_encode(pack_mask_bits(d), width=W), rle_encode(d.to(torch.uint8) * 255)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host(device, name):
    mask = CASES[name]
    want = rle_encode(mask)
    for got in _device_both_forms(mask, device):
        assert got == want


def test_large_zero_count_takes_five_characters(device):
    got = rle_encode(CASES["1056x1000_zero"].to(device))
    assert len(got[0]["counts"]) == 5 and got == rle_encode(CASES["1056x1000_zero"])


def test_planes_in_one_call(device):
    """Five planes, an all-zero one between two busy ones: the per-mask offsets."""
    masks = torch.stack([_rand((19, 45), 0.5, 1), _checker(19, 45), torch.zeros(19, 45, dtype=torch.bool),
                         _rand((19, 45), 0.5, 2), torch.ones(19, 45, dtype=torch.bool)])
    want = rle_encode(masks)
    assert len(want) == 5 and want[2]["counts"] == rle_encode(torch.zeros(19, 45, dtype=torch.bool))[0]["counts"]
    for got in _device_both_forms(masks, device):
        assert got == want
    four_d = masks[None].expand(2, 5, 19, 45).contiguous()
    assert rle_encode(four_d.to(device)) == want + want


def test_crop_view_is_read_in_place(device):
    big = _rand((3, 40, 80), 0.5, 3)
    crop = big.to(device)[:, 2:35, 3:68]
    assert not crop.is_contiguous() and crop.stride() == (3200, 80, 1)
    want = rle_encode(big[:, 2:35, 3:68])
    assert rle_encode(crop) == want
    assert rle_encode(crop.to(torch.uint8)[:, :, :]) == want


def test_two_calls_give_identical_bytes(device):
    masks = torch.stack([_rand((33, 65), 0.5, 4), _checker(33, 65)]).to(device)
    bits = pack_mask_bits(masks)
    assert rle_encode(masks) == rle_encode(masks)
    assert rle_encode(bits, width=65) == rle_encode(bits, width=65)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_video_head_rle(device, dtype):
    Q, K, T = 12, 5, 3
    g = torch.Generator().manual_seed(0)
    out = {"pred_logits": (torch.randn(1, Q, K + 1, generator=g) * 2).to(device),
           "pred_masks": (torch.randn(1, Q, T, 20, 28, generator=g) * 3).to(device, dtype)}
    head = VideoMaskFormerInference(K)
    args = (out, (80, 112), (75, 100), (90, 130))
    plain, enc = head(*args, packed=False), head(*args, rle=True)
    assert enc["rle"] is True and enc["image_size"] == (90, 130)
    assert enc["pred_scores"] == plain["pred_scores"] and enc["pred_labels"] == plain["pred_labels"]
    assert len(enc["pred_masks"]) == len(plain["pred_masks"]) == 10
    for e, m in zip(enc["pred_masks"], plain["pred_masks"]):
        assert len(e) == T and e == rle_encode(m)


def test_image_head_instance_rle(device):
    B, Q, K = 2, 12, 5
    g = torch.Generator().manual_seed(1)
    out = {"pred_logits": (torch.randn(B, Q, K + 1, generator=g) * 2).to(device),
           "pred_masks": (torch.randn(B, Q, 16, 24, generator=g) * 3).to(device)}
    head = MaskFormerInference(num_classes=K, semantic_on=False, instance_on=True, test_topk_per_image=20)
    args = (out, (64, 96), [(60, 90), (64, 70)], [(45, 67), (64, 70)])
    plain, enc = head(*args), head(*args, instance_rle=True)
    for b, size in enumerate([(45, 67), (64, 70)]):
        p, e = plain[b]["instances"], enc[b]["instances"]
        assert "pred_masks" not in e
        assert len(e["pred_masks_rle"]) == 20 and e["pred_masks_rle"][0]["size"] == list(size)
        assert e["pred_masks_rle"] == rle_encode((p["pred_masks"] > 0).cpu())
        assert e["image_size"] == size
        for k in ("scores", "pred_classes", "pred_boxes"):
            assert torch.equal(e[k], p[k])
