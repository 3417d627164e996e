"""The box-supervised video criterion on the device (bm2f_amd/video_criterion.py, csrc/video_pairs.hip via
bm2f_amd/weaksup.py) against the reference's outputs (tests/golden/video_criterion.npz) and fp64 autograd of the
reference formula.

Bars: matched indices exact; losses rtol 1e-5, gradients rtol 1e-4 (fp32 sums in another order); the temporal
kernel value rtol 1e-5, gradient rtol 1e-4 / atol 1e-6, two backward runs bit-identical; mining: counts and
current-pixel order exact, the chosen next pixel within one fp16 ulp (2^-9 relative) plus the reference's measured
cdist error of the fp64 minimum, and equal to the reference's choice wherever only one pixel is admissible."""
import os

import numpy as np
import pytest
import torch

from bm2f_amd import weaksup
from test_video_criterion_cpu import check_against_fixture, check_mining, fixture_targets, to_device

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "video_criterion.npz"))


_runs = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_target"])
def test_criterion_vs_reference(device, gold, shared, dtype):
    """The fixture's mask logits are exact in fp16, so both dtypes must reproduce the reference."""
    targets = to_device(fixture_targets(gold, shared=False), device)
    if shared:
        targets = [dict(t, color_similarities=t["color_similarities"][:1].expand_as(t["color_similarities"]))
                   for t in targets]
    _runs[(shared, dtype)] = check_against_fixture(gold, device, targets, mask_dtype=dtype)
    other = _runs.get((not shared, dtype))
    if other is not None:       # the two similarity paths agree with each other too (indices are checked above)
        for a, b in zip(_runs[(shared, dtype)], other):
            for k in a:
                np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-7, err_msg=k)


def _random_pairs(g, T, H, W, counts):
    """counts[row][t] pairs per (target row, frame pair), with repeated endpoints on both sides."""
    clip = []
    for per in counts:
        frames = []
        for k in per:
            cur = torch.stack([torch.randint(0, W, (k,), generator=g), torch.randint(0, H, (k,), generator=g)], 1)
            nxt = torch.stack([torch.randint(0, W, (k,), generator=g), torch.randint(0, H, (k,), generator=g)], 1)
            if k >= 8:
                nxt[: k // 2] = nxt[0]            # many-to-one: half the pairs end on one pixel
                cur[k // 2:k // 2 + 3] = cur[-1]  # one-to-many
            frames.append((cur.int(), nxt.int()))
        clip.append(frames)
    return clip


def _reference_sum(x, rows, clip):
    """fp64 restatement of loss_temporal_pairwise's sum (criterion_proj_spatpair_temppair.py:38-69, :289-318)."""
    total, count = x.new_zeros(()), 0
    for g, n in enumerate(rows):
        if n < 0:
            continue
        for t, (cur, nxt) in enumerate(clip[g]):
            a = x[n, t][cur[:, 1].long(), cur[:, 0].long()]
            b = x[n, t + 1][nxt[:, 1].long(), nxt[:, 0].long()]
            total = total + weaksup._pair_term_torch(a, b).sum()
            count += cur.shape[0]
    return total, count


def test_temporal_kernel_vs_fp64(device):
    N, T, H, W = 3, 3, 17, 45
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, T, H, W, generator=g) * 4
    x[0, :, :4, :6] = 40.0                                     # saturated logits, both signs
    x[1, :, 5:9, 10:30] = -40.0
    # 5 targets: one with zero pairs, one unmatched (row_of_target -1); more than one block of pairs
    counts = [[300, 40], [0, 0], [25, 0], [64, 64], [130, 7]]
    rows = [2, 0, -1, 1, -1]
    clip = _random_pairs(g, T, H, W, counts)
    clip[0][0][0][:10] = torch.tensor([2, 1])                  # pairs inside the +40 patch ...
    clip[0][0][1][:5] = torch.tensor([3, 2])
    clip[3][1][0][:6] = torch.tensor([15, 6])                  # ... and the -40 patch, and mixed-sign pairs
    clip[3][1][1][:6] = torch.tensor([1, 1])
    pk = weaksup.pack_temporal_pairs([clip], T, H, W, device)
    rot = torch.tensor(rows, dtype=torch.int32, device=device)
    xd = x.clone().to(device).requires_grad_()
    total, count = weaksup.temporal_pair_sum(xd, rot, pk)
    scale = 0.37
    (total * scale).backward()
    x64 = x.double().requires_grad_()
    want, n_want = _reference_sum(x64, rows, clip)
    (want * scale).backward()
    assert int(count) == n_want
    print(f"temporal sum: got {float(total.detach()):.9g} want {float(want):.9g}; max |grad err| "
          f"{float((xd.grad.cpu().double() - x64.grad).abs().max()):.3e}")
    assert torch.isfinite(total)
    np.testing.assert_allclose(float(total), float(want), rtol=1e-5)
    torch.testing.assert_close(xd.grad.cpu().double(), x64.grad, rtol=1e-4, atol=1e-6)
    assert (xd.grad.cpu()[x64.grad == 0] == 0).all()           # untouched pixels are exactly zero
    first = xd.grad.clone()
    xd.grad = None
    total2, _ = weaksup.temporal_pair_sum(xd, rot, pk)
    (total2 * scale).backward()
    assert torch.equal(first, xd.grad) and torch.equal(total, total2)   # no atomics: bitwise repeatable


def test_temporal_term_equals_spatial_term(device):
    """The temporal and the spatial loss evaluate one pair_term (csrc/device_util.h): on the same two logits they
    give the same fp32 value.  Both frames of a clip hold one plane, so the temporal pair (pixel (y, x) of frame 0,
    pixel (y, x + 1) of frame 1) is the spatial pair of (y, x) with its right-hand neighbour (tap 4, dilation 1).
    One pair per launch: the block reduction then adds only zeros to the term, so the sum is the term itself (a
    -0 term sums to +0: compared as values) and the comparison is exact (same expression, same compile flags: no
    tolerance to grant)."""
    H, W = 5, 9
    g = torch.Generator().manual_seed(3)
    plane = torch.randn(H, W, generator=g) * 4
    plane[0, :4] = torch.tensor([40.0, 40.0, -40.0, -40.0])   # saturated: ++, +-, --
    plane[1, :3] = torch.tensor([0.0, 0.0, 1e-3])
    x = plane.expand(1, 2, H, W).contiguous().to(device)
    spatial = weaksup.pairwise_planes(x[0, :1].contiguous(), 1)[0, 4].cpu()
    rot = torch.zeros(1, dtype=torch.int32, device=device)
    for y, xx in [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 3), (4, 7)]:
        cur, nxt = torch.tensor([[xx, y]], dtype=torch.int32), torch.tensor([[xx + 1, y]], dtype=torch.int32)
        pk = weaksup.pack_temporal_pairs([[[(cur, nxt)]]], 2, H, W, device)
        total, count = weaksup.temporal_pair_sum(x, rot, pk)
        print(f"pair ({y}, {xx}): temporal {float(total):.9g} spatial {float(spatial[y, xx]):.9g}")
        assert int(count) == 1 and float(total) == float(spatial[y, xx]) and float(total) >= 0.0


def test_temporal_kernel_no_pairs(device):
    T, H, W = 3, 17, 45
    e = torch.zeros((0, 2), dtype=torch.int64)
    pk = weaksup.pack_temporal_pairs([[[(e, e), (e, e)]]], T, H, W, device)
    assert pk.P == 0
    x = torch.randn(1, T, H, W, device=device, requires_grad=True)
    total, count = weaksup.temporal_pair_sum(x, torch.zeros(1, dtype=torch.int32, device=device), pk)
    assert float(total) == 0.0 and int(count) == 0
    (total / count.float().clamp(min=1.0)).backward()
    assert x.grad is not None and not x.grad.any()


def test_mining_vs_reference(device, gold):
    """Boxes up to 12 x 9 (two 64-pixel tiles of current pixels), a 1 x 1 box, a box on the frame edge and a
    zero-area box (the fixture's clip 0)."""
    check_mining(gold, device)


def test_mining_packed_form_feeds_the_loss(device, gold):
    """MinedPairs goes into the criterion's packing as is and equals its own nested-list form."""
    z = gold
    T, H, W = (int(z[k]) for k in ("T", "H", "W"))
    feats = torch.from_numpy(z["feats0"]).float().to(device) / float(z["feat_scale"])
    mined = weaksup.temporal_pairs(feats, torch.from_numpy(z["boxes0"]).to(device))
    a = weaksup.pack_temporal_pairs([mined], T, H, W, device)
    b = weaksup.pack_temporal_pairs([mined.to_lists()], T, H, W, device)
    for k in ("row", "t", "p0", "p1", "ep_key", "ep_code"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.P == sum(sum(r) for r in mined.counts) and not bool(a.bad)
