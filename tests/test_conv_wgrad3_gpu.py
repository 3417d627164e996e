"""The tap-fused 3x3 weight gradient (csrc/conv_x3.hip x3_conv_wgrad3_fused_kernel, conv_ops.wgrad3_fused) against fp64
F.conv2d at the x3 engine's bound (relative Frobenius error < 2e-6, as test_conv_x3_vs_fp64), on the smallest shapes at
which it can go wrong: one chunk wide maps (every staged row touches both borders), channel counts that are no multiple
of the 128 x 32 block tile, slabs that end inside an image, several slabs per tile; exact border counts; bitwise
repeatability; agreement with the "tn" route."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from bm2f_amd import conv_ops

pytestmark = pytest.mark.gpu

BOUND = 2e-6   # the x3 engine's bound (tests/test_conv_gpu.py)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _ref(g, x):
    """fp64 weight and bias gradient of a 3x3 "same" conv."""
    Co, Ci = g.shape[1], x.shape[1]
    w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, device=x.device, requires_grad=True)
    b = torch.zeros(Co, dtype=torch.float64, device=x.device, requires_grad=True)
    F.conv2d(x.double(), w, b, padding=1).backward(g.double())
    return w.grad, b.grad


SHAPES = [(1, 16, 16, 16, 8, False), (1, 48, 16, 128, 8, False), (2, 16, 32, 16, 8, True), (3, 32, 48, 8, 16, True),
          (2, 256, 256, 32, 32, False)]


@pytest.mark.parametrize("N,Ci,Co,H,W,bias", SHAPES)
def test_wgrad3_fused_vs_fp64(device, N, Ci, Co, H, W, bias, monkeypatch):
    """Through Conv2dX3.backward with WGRAD3 = "fused" (the library's own slab count)."""
    monkeypatch.setattr(conv_ops, "WGRAD3", "fused")
    torch.manual_seed(Ci + Co + H)
    conv = nn.Conv2d(Ci, Co, 3, padding=1, bias=bias).to(device)
    x = torch.randn(N, Ci, H, W, device=device, requires_grad=True)
    assert conv_ops.eligible(x, conv)
    y = conv_ops.conv2d(x, conv)
    g = torch.randn_like(y)
    y.backward(g)
    dw, db = _ref(g, x.detach())
    assert conv.weight.grad.shape == (Co, Ci, 3, 3)
    assert _rel(conv.weight.grad, dw) < BOUND
    if bias:
        assert _rel(conv.bias.grad, db) < BOUND


@pytest.mark.parametrize("N,Ci,Co,H,W,splits", [(1, 16, 16, 16, 8, 4), (3, 32, 48, 8, 16, 5), (3, 32, 48, 8, 16, 2),
                                                (2, 16, 32, 16, 8, 3), (1, 48, 16, 128, 8, 7),
                                                (1, 16, 16, 6, 64, 3)])
def test_wgrad3_fused_forced_slabs(device, N, Ci, Co, H, W, splits):
    """More than one slab per tile, forced through the entry point's splits argument: slabs of one chunk (4 chunks in
    4 slabs), slabs that end and start inside different images (12 chunks in 5 and in 2 slabs), a slab count that
    does not divide the chunks; H = 6: a last chunk row of which only two rows are inside the image."""
    torch.manual_seed(N * 7 + splits)
    x = torch.randn(N, Ci, H, W, device=device)
    g = torch.randn(N, Co, H, W, device=device)
    dw, db = conv_ops.wgrad3_fused(g, x, True, splits=splits)
    rw, rb = _ref(g, x)
    assert _rel(dw, rw) < BOUND
    assert _rel(db, rb) < BOUND


def test_wgrad3_fused_border_mask_exact(device):
    """dO nonzero (= 1) only in the four corners and the four edge midpoints, I all ones: a tap's gradient is the number
    of those pixels whose shifted partner lies inside the image, a small integer, exactly."""
    N, Ci, Co, H, W = 2, 16, 16, 8, 16
    g = torch.zeros(N, Co, H, W, device=device)
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    for y, x_ in pts:
        g[:, :, y, x_] = 1.0
    x = torch.ones(N, Ci, H, W, device=device)
    dw, db = conv_ops.wgrad3_fused(g, x, True)
    want = torch.zeros(3, 3)
    for ky in range(3):
        for kx in range(3):
            want[ky, kx] = N * sum(0 <= y + ky - 1 < H and 0 <= x_ + kx - 1 < W for y, x_ in pts)
    assert torch.equal(dw.cpu(), want.expand(Co, Ci, 3, 3))
    assert torch.equal(db.cpu(), torch.full((Co,), float(N * len(pts))))


def test_wgrad3_fused_border_input(device):
    """I nonzero only in the border rows and columns (every product crosses a zeroed halo or sits next to one)."""
    N, Ci, Co, H, W = 2, 32, 16, 16, 24
    torch.manual_seed(3)
    x = torch.randn(N, Ci, H, W, device=device)
    x[:, :, 1:H - 1, 1:W - 1] = 0.0
    g = torch.randn(N, Co, H, W, device=device)
    dw, _ = conv_ops.wgrad3_fused(g, x, False, splits=3)
    rw, _ = _ref(g, x)
    assert _rel(dw, rw) < BOUND


def test_wgrad3_fused_bitwise_repeatable(device):
    torch.manual_seed(5)
    x = torch.randn(3, 48, 16, 16, device=device)
    g = torch.randn(3, 144, 16, 16, device=device)
    a = conv_ops.wgrad3_fused(g, x, True)
    b = conv_ops.wgrad3_fused(g, x, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wgrad3_fused_matches_tn_route(device):
    """The two engines sum in different orders: equal within the engine's bound, not bitwise."""
    torch.manual_seed(9)
    x = torch.randn(2, 64, 16, 32, device=device)
    g = torch.randn(2, 48, 16, 32, device=device)
    dw, db = conv_ops.wgrad3_fused(g, x, True)
    tn = conv_ops._wgrad3_tn(g, x)
    assert _rel(dw, tn) < BOUND
    assert _rel(db, g.sum((2, 3)).sum(0)) < BOUND
