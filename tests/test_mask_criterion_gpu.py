"""The mask-supervised matcher and criterion on the device (bm2f_amd/mask_criterion.py, csrc/point_sample.hip)
against the reference's outputs (tests/golden/mask_criterion.npz) and, kernel by kernel, against an fp64 torch
restatement.

Bars: the fixture check keeps the CPU test's bars (indices and kept sets exact, losses rtol 1e-5, gradients rtol
1e-4 / atol 1e-6; fp16 masks: gradient rtol 2^-10, the rounding of the gradient to fp16).  Each kernel alone: the
error against fp64 is at most twice the error of fp32 ``F.grid_sample`` (the reference's own op, run on the CPU) on
the same inputs, with a floor of 1e-6 of the tensor's maximum; both are measured here.  The match cost is bitwise
repeatable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bm2f_amd import mask_criterion as mc
from test_mask_criterion_cpu import (check_against_fixture, check_box_mask_type, check_empty_cases, fixture_targets,
                                     gold)  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("tdtype", [torch.bool, torch.float32], ids=["bool", "float"])
@pytest.mark.parametrize("case", ["img", "vid"])
def test_criterion_vs_reference(device, gold, case, tdtype, dtype):  # noqa: F811
    """The fixture's mask logits are exact in fp16, so both dtypes must reproduce the reference."""
    targets = [{k: v.to(device) for k, v in t.items()} for t in fixture_targets(gold, case, tdtype)]
    check_against_fixture(gold, case, device, targets, mask_dtype=dtype,
                          grad_rtol=1e-4 if dtype == torch.float32 else 2.0 ** -10)


@pytest.mark.parametrize("case", ["img", "vid"])
def test_empty_cases(device, gold, case):  # noqa: F811
    check_empty_cases(gold, case, device)


def test_box_mask_target_type(device, gold):  # noqa: F811
    check_box_mask_type(gold, device)


# ------------------------------------------------------------------------------------------------------------
# kernels alone
# ------------------------------------------------------------------------------------------------------------
def _coords(g, rows, K, H, W):
    """(rows, K, 2) in [0, 1): uniform, plus exactly 0, the largest float below 1 and points within half a pixel of
    each border (where one or two corners fall outside the plane)."""
    u = torch.rand(rows, K, 2, generator=g)
    top = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    u[:, 0] = torch.tensor([0.0, 0.0])
    u[:, 1] = torch.tensor([top, top])
    u[:, 2] = torch.tensor([0.0, top])
    u[:, 3] = torch.tensor([0.25 / W, 0.5])                    # within half a pixel of the left border
    u[:, 4] = torch.tensor([1.0 - 0.25 / W, 0.3])              # ... the right
    u[:, 5] = torch.tensor([0.4, 0.3 / H])                     # ... the top
    u[:, 6] = torch.tensor([0.6, 1.0 - 0.3 / H])               # ... the bottom
    u[:, 7] = torch.tensor([0.5 / W, 1.0 - 0.5 / H])           # exactly on the first / last pixel centre
    return u


def _bar(ref32, ref64):
    """Twice the fp32 CPU restatement's distance from fp64, floored at 1e-6 of the tensor's maximum."""
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    return max(2.0 * float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0, 1e-6 * scale)


def _check(name, got, ref32, ref64):
    bar = _bar(ref32, ref64)
    err = float((got.double().cpu() - ref64).abs().max()) if ref64.numel() else 0.0
    print(f"{name}: err {err:.3e} bar {bar:.3e} (fp32 torch err {bar / 2:.3e}, max {float(ref64.abs().max()) if ref64.numel() else 0:.3e})")
    assert err <= bar, (name, err, bar)


def _match_ref(masks, tgts, coords, weights, cls, dtype):
    """The matcher's cost per image in `dtype` on the CPU: (B, Q, Gm), padding columns 0."""
    B, Q = masks.shape[:2]
    Gm = max(t.shape[0] for t in tgts)
    wc, wm, wd = weights
    C = torch.zeros(B, Q, Gm, dtype=dtype)
    for b in range(B):
        G = tgts[b].shape[0]
        if G == 0:
            continue
        x, t = masks[b].to(dtype), tgts[b].to(dtype)
        if x.dim() == 3:
            x, t = x[:, None], t[:, None]
        u = coords[b:b + 1].to(dtype)
        x = mc.point_sample(x, u.expand(Q, -1, -1)).flatten(1)
        t = mc.point_sample(t, u.expand(G, -1, -1)).flatten(1)
        s = x.sigmoid()
        cm = (F.softplus(x).sum(1)[:, None] - x @ t.t()) / x.shape[1]
        cd = 1 - (2 * (s @ t.t()) + 1) / (s.sum(1)[:, None] + t.sum(1)[None] + 1)
        C[b, :, :G] = wm * cm + wc * cls[b, :, :G].to(dtype) + wd * cd
    return C


MATCH_SHAPES = [  # H, W, K, Q, G per image, T (0: image)
    (20, 28, 50, 12, [4, 0, 1], 0),
    (7, 5, 130, 12, [1, 4, 0], 0),
    (20, 28, 130, 12, [4, 1], 3),
    (7, 5, 50, 12, [0, 4], 3),
    (7, 5, 300, 40, [35, 2], 0),      # two point tiles, two query chunks, two target chunks
]


@pytest.mark.parametrize("tdtype", [torch.bool, torch.float32], ids=["bool", "float"])
@pytest.mark.parametrize("shape", MATCH_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + f"T{s[5]}")
def test_match_cost_kernel_vs_fp64(device, shape, tdtype):
    H, W, K, Q, Gs, T = shape
    g = torch.Generator().manual_seed(H * 1000 + K + T)
    B = len(Gs)
    lead = (B, Q, T) if T else (B, Q)
    masks = torch.randn(*lead, H, W, generator=g) * 4
    tgts = [(torch.rand(*((G, T) if T else (G,)), 4 * H, 4 * W, generator=g) > 0.6) for G in Gs]
    if tdtype == torch.float32:
        tgts = [t.float() * torch.rand(t.shape, generator=g) for t in tgts]       # soft targets
    coords = _coords(g, B, K, H, W)
    Gm = max(Gs)
    cls = -torch.rand(B, Q, Gm, generator=g)
    weights = (2.0, 5.0, 3.0)
    tg = mc.MaskTargets([{"labels": torch.zeros(G, dtype=torch.int64), "masks": t} for G, t in zip(Gs, tgts)], device,
                        bool(T))
    pl = tg.planes("masks")
    assert pl["code"] == (0 if tdtype == torch.bool else 1)
    args = (masks.to(device), coords.to(device), pl["match"], pl["code"], Gm, cls.to(device), *weights)
    got = mc.match_cost(*args)
    again = mc.match_cost(*args)
    assert torch.equal(got, again)                                   # fixed-order reduction: bit-identical
    for b, G in enumerate(Gs):
        assert not got[b, :, G:].any()
    _check("match cost", got, _match_ref(masks, tgts, coords, weights, cls, torch.float32),
           _match_ref(masks, tgts, coords, weights, cls, torch.float64))


def _rows_case(g, H, W, K, device, tdtype):
    """R = 5 rows over 3 x 4 planes; row targets at 4x resolution, one normalised over a larger (padded) extent."""
    masks = torch.randn(3, 4, H, W, generator=g) * 4
    plane = torch.tensor([7, 0, 11, 7, 2], dtype=torch.int64)
    R = plane.shape[0]
    sizes = [(4 * H, 4 * W)] * (R - 1) + [(3 * H, 3 * W + 1)]
    tgts = [(torch.rand(h, w, generator=g) > 0.5) for h, w in sizes]
    if tdtype == torch.float32:
        tgts = [t.float() * torch.rand(t.shape, generator=g) for t in tgts]
    else:
        tgts = [t.view(torch.uint8) for t in tgts]
    coords = _coords(g, R, K, H, W)
    dev_t = [t.to(device).contiguous() for t in tgts]
    rows = torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], 4 * H, 4 * W] for t in dev_t], dtype=torch.int64)
    padded = torch.stack([F.pad(t.float(), (0, 4 * W - t.shape[1], 0, 4 * H - t.shape[0])) for t in tgts])
    return masks, plane, coords, dev_t, rows.to(device), padded


def _rows_ref(masks, plane, coords, padded, dtype, grads=None):
    m = masks.detach().to(dtype).clone().requires_grad_()
    x = mc.point_sample(m.flatten(0, 1)[plane][:, None], coords.to(dtype))[:, 0]
    t = mc.point_sample(padded.to(dtype)[:, None], coords.to(dtype))[:, 0]
    s = x.sigmoid()
    out = [F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1), (s * t).sum(1), s.sum(1), t.sum(1)]
    gm = None
    if grads is not None:
        sum((o * gr.to(dtype)).sum() for o, gr in zip(out[:3], grads)).backward()
        gm = m.grad
    return [o.detach() for o in out], -x.detach().abs(), gm


@pytest.mark.parametrize("tdtype", [torch.bool, torch.float32], ids=["bool", "float"])
@pytest.mark.parametrize("hwk", [(20, 28, 50), (7, 5, 130), (7, 5, 1100)], ids=lambda s: "x".join(map(str, s)))
def test_row_kernels_vs_fp64(device, hwk, tdtype):
    """Uncertainty, loss forward and loss backward (K = 1100: two chunks of the forward's partials)."""
    H, W, K = hwk
    g = torch.Generator().manual_seed(H + K)
    masks, plane, coords, keep, rows, padded = _rows_case(g, H, W, K, device, tdtype)
    grads = [torch.randn(plane.shape[0], generator=g) for _ in range(3)]
    s32, u32, g32 = _rows_ref(masks, plane, coords, padded, torch.float32, grads)
    s64, u64, g64 = _rows_ref(masks, plane, coords, padded, torch.float64, grads)
    md = masks.to(device).requires_grad_()
    _check("uncertainty", mc.point_uncertainty(md.detach(), plane.to(device), coords.to(device)), u32, u64)
    code = 0 if tdtype == torch.bool else 1
    out = mc.point_loss_sums(md, plane.to(device), coords.to(device), rows, code, keep=keep)
    for name, got, a, b in zip(("bce", "sum sig t", "sum sig", "sum t"), out, s32, s64):
        _check(name, got.detach(), a, b)
    sum((o * gr.to(device)).sum() for o, gr in zip(out[:3], grads)).backward()
    _check("grad", md.grad, g32, g64)
    assert not md.grad.cpu()[g64 == 0].any()                          # untouched pixels stay exactly zero
    # a row whose plane index is out of range is skipped, not read
    bad = plane.clone()
    bad[1] = 12
    out = mc.point_loss_sums(md.detach(), bad.to(device), coords.to(device), rows, code, keep=keep)
    assert all(float(o[1]) == 0.0 for o in out)
