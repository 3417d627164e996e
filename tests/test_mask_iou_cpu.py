"""bm2f_amd.mask_iou on the host (no GPU): rle_to_bits against pack_mask_bits(rle_decode(...)) in the three forms of
``counts``, its ValueErrors, mask_pair_counts and mask_iou against dense numpy definitions, and the argument checks
of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from bm2f_amd import (_native, mask_iou, mask_pair_counts, pack_mask_bits, rle_decode, rle_encode, rle_to_bits,
                      string_to_counts)
from bm2f_amd.mask_iou import pair_tiles


def _forms(rles):
    """The same masks with compressed str, compressed bytes and uncompressed list counts."""
    return (rles,
            [None if r is None else dict(r, counts=r["counts"].encode("ascii")) for r in rles],
            [None if r is None else dict(r, counts=string_to_counts(r["counts"])) for r in rles])


@pytest.mark.parametrize("size", [(1, 1), (7, 31), (33, 65), (5, 64), (40, 33)])
@pytest.mark.parametrize("p", [0.02, 0.5, 0.98])
def test_rle_to_bits_equals_decode(size, p):
    H, W = size
    g = torch.Generator().manual_seed(H * 100 + W + int(p * 10))
    masks = torch.rand(6, H, W, generator=g) < p
    masks[0] = False
    masks[1] = True
    masks[2] = False
    masks[2, 0, 0] = True                                             # pixel 0: counts start with a zero
    masks[3, -1, -1] = True
    rles = rle_encode(masks)
    rles = rles[:2] + [None] + rles[2:] + [None]
    want = torch.stack([torch.zeros(H, (W + 31) // 32, dtype=torch.int32) if r is None
                        else pack_mask_bits(rle_decode(r)) for r in rles])
    for form in _forms(rles):
        got = rle_to_bits(form)
        assert got.dtype == torch.int32 and torch.equal(got, want)
    mixed = [f[i] for i, f in zip(range(len(rles)), _forms(rles) * 3)]
    assert torch.equal(rle_to_bits(mixed), want)


def test_rle_to_bits_sizes_and_empty_inputs():
    assert tuple(rle_to_bits([None, None], size=(5, 40)).shape) == (2, 5, 2)
    assert rle_to_bits([None], size=(5, 40)).abs().sum() == 0
    assert tuple(rle_to_bits([], size=(5, 40)).shape) == (0, 5, 2)
    with pytest.raises(ValueError):
        rle_to_bits([None])
    with pytest.raises(ValueError):
        rle_to_bits([])


def test_rle_to_bits_value_errors():
    ok = rle_encode(torch.ones(4, 4, dtype=torch.bool))[0]
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 4], "counts": [3, 5, 7]}])          # sums to 15
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 4], "counts": [20, -4]}])           # negative
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 5], "counts": ok["counts"]}])       # 16 pixels in a 4 x 5 mask
    with pytest.raises(ValueError):
        rle_to_bits([ok, {"size": [5, 4], "counts": [20]}])           # two sizes
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 4], "counts": ""}])
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 4], "counts": "`"}])                # ends inside a value
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [4, 4], "counts": "0 0"}])              # a character below '0'
    with pytest.raises(ValueError):
        rle_to_bits([{"size": [1 << 16, 1 << 15], "counts": [1 << 31]}])
    assert rle_to_bits([{"size": [4, 4], "counts": [0, 16]}]).tolist() == [[[15]] * 4]


def _dense_counts(a, b):
    inter = (a[:, None] & b[None]).sum((2, 3, 4)).numpy()
    return inter, a.sum((2, 3)).numpy(), b.sum((2, 3)).numpy()


@pytest.mark.parametrize("width", [1, 31, 32, 33, 70])
def test_pair_counts_host_equals_dense(width):
    g = torch.Generator().manual_seed(width)
    a = torch.rand(3, 2, 9, width, generator=g) < 0.5
    b = torch.rand(2, 2, 9, width, generator=g) < 0.3
    pa, pb = pack_mask_bits(a), pack_mask_bits(b)
    for got in (mask_pair_counts(pa, pb, width), mask_pair_counts(pa | _tail(width), pb | _tail(width), width)):
        for x, y in zip(got, _dense_counts(a, b)):
            assert x.dtype == np.int64 and np.array_equal(x, y)
    inter, area_a, area_b = mask_pair_counts(pa[:0], pb, width)
    assert inter.shape == (0, 2) and area_a.shape == (0, 2) and np.array_equal(area_b, b.sum((2, 3)).numpy())
    with pytest.raises(ValueError):
        mask_pair_counts(pa, pb[:, :1], width)
    with pytest.raises(ValueError):
        mask_pair_counts(pa, pb, width + 32)


def _tail(width):
    """A word with every bit beyond ``width`` set (0 when the width fills its last word)."""
    r = width % 32
    v = 0 if r == 0 else ((1 << 32) - (1 << r))
    return torch.tensor(v - (1 << 32) if v >= 1 << 31 else v, dtype=torch.int32) * _last_word(width)


def _last_word(width):
    m = torch.zeros((width + 31) // 32, dtype=torch.int32)
    m[-1] = 1
    return m


def test_mask_iou_against_dense_definition():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(4, 2, 6, 40, generator=g) < 0.5
    b = torch.rand(3, 2, 6, 40, generator=g) < 0.5
    a[3] = False
    b[2] = False                                                      # the pair (3, 2) has union 0
    inter, area_a, area_b = mask_pair_counts(pack_mask_bits(a), pack_mask_bits(b), 40)
    i = (a[:, None] & b[None]).sum((2, 3, 4)).double().numpy()
    u = (a[:, None] | b[None]).sum((2, 3, 4)).double().numpy()
    want = np.where(u > 0, i / np.maximum(u, 1), 0.0)
    got = mask_iou(inter, area_a, area_b)
    assert got.dtype == np.float64 and np.array_equal(got, want) and got[3, 2] == 0.0
    assert np.array_equal(mask_iou(inter, area_a.sum(1), area_b.sum(1)), want)
    crowd = [False, True, True]
    area = a.sum((1, 2, 3)).double().numpy()[:, None]
    want_crowd = np.where(np.array(crowd)[None], np.where(area > 0, i / np.maximum(area, 1), 0.0), want)
    got_crowd = mask_iou(inter, area_a, area_b, iscrowd=crowd)
    assert np.array_equal(got_crowd, want_crowd) and got_crowd[3, 1] == 0.0
    one, two = np.array([[1]]), np.array([[1]])
    assert mask_iou(one, two, np.array([[2]]))[0, 0] == 0.5           # intersection 1 of union 2


def test_tile_constants():
    ta, tb, chunk = pair_tiles()
    assert ta >= 1 and tb >= 1 and chunk >= 256 and chunk % 4 == 0


def test_c_entry_argument_checks():
    """Refused before any HIP call: the fake pointers never reach a kernel."""
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 2)
    L = ctypes.c_int64
    nbytes = L()
    rc = lib.m2f_rle_decode_bits(p, L(4), None, 1, 4, 4, p, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_decode_bits(None, L(4), p, 1, 4, 4, p, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_rle_decode_bits(p, L(4), p, 0, 4, 4, p, None)
    assert rc == 1 and b"positive" in lib.m2f_last_error()
    rc = lib.m2f_rle_decode_bits(p, L(4), p, 1, 1 << 16, 1 << 15, p, None)
    assert rc == 1 and b"32-bit" in lib.m2f_last_error()
    rc = lib.m2f_rle_decode_bits(p, L(4), odd, 1, 4, 4, p, None)
    assert rc == 1 and b"aligned" in lib.m2f_last_error()
    rc = lib.m2f_rle_decode_bits(p, L(4), p, 70000, 4, 4, p, None)
    assert rc == 3
    rc = lib.m2f_bits_pair_workspace(2, 2, 2, 300, 700, None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_workspace(0, 2, 2, 300, 700, ctypes.byref(nbytes))
    assert rc == 1 and b"positive" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_workspace(2, 2, 70000, 4, 4, ctypes.byref(nbytes))
    assert rc == 3
    assert lib.m2f_bits_pair_workspace(2, 2, 2, 300, 700, ctypes.byref(nbytes)) == 0
    ta, tb, chunk = pair_tiles()
    chunks = -(-300 * 22 // chunk)
    assert nbytes.value == 1 * 1 * 2 * chunks * (ta * tb + ta + tb) * 4 and chunks > 1
    n = 2 * 300 * 22
    args = (p, 2, L(n), p, 2, L(n), 2, 300, 700, p, p, p, p, L(nbytes.value), None)
    rc = lib.m2f_bits_pair_counts(None, *args[1:])
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(*args[:12], None, L(nbytes.value), None)
    assert rc == 1 and b"null" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(p, 2, L(n - 1), *args[3:])
    assert rc == 1 and b"stride" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(*args[:5], L(n - 1), *args[6:])
    assert rc == 1 and b"stride" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(*args[:13], L(nbytes.value - 1), None)
    assert rc == 1 and b"workspace" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(odd, *args[1:])
    assert rc == 1 and b"aligned" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(*args[:9], ctypes.c_void_p((1 << 20) + 4), *args[10:])
    assert rc == 1 and b"aligned" in lib.m2f_last_error()
    rc = lib.m2f_bits_pair_counts(*args[:7], 1 << 16, 1 << 15, *args[9:])
    assert rc == 1 and b"32-bit" in lib.m2f_last_error()
    assert lib.m2f_bits_pair_tiles(None, None, None) == 1
    pair_tiles()                                                       # a success clears the message
    assert lib.m2f_last_error() == b""
