"""Semantic test-time augmentation on the GPU (csrc/semantic_tta.hip through semantic_inference_tta): the case of
tests/golden/tta.npz in both orders and three logit dtypes, class / query edges, a single view against the existing
fused head, the mirrored column index, the global-load fallback, determinism, peak memory in labels mode and the driver.

fp32 logits are held to the reference's results in the fixture; everything else to the CPU path (for 16-bit logits
on ``logits.float()``, the definition of correct for them, csrc/resize_device.h).  Bars: tta_util.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import inference_util as iu
import tta_util as tu

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _run(views, output, device, before, dtype=None, **kw):
    from bm2f_amd import semantic_inference_tta
    K = views[0]["cls"].shape[1] - 1
    return semantic_inference_tta(tu.api_views(views, device, dtype), output, num_classes=K, before=before, **kw)


def _rounded(views, dtype):
    return [dict(v, masks=v["masks"].to(dtype).float()) for v in views]


@functools.lru_cache(maxsize=None)
def _expected(order, dt):
    c = tu.load()
    if dt == "fp32":
        return tu.expected_fixture(order)
    return tu.expected_from_cpu(_rounded(c.views, DTYPES[dt]), c.output, order == "before")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("order", tu.ORDERS)
def test_fixture_case(order, dt, device):
    """Output 37 x 53 (odd width, no multiple of the 4 x 32 tile), V = 4 (two scales x flip), Q = 20, K = 19."""
    c = tu.load()
    e = _expected(order, dt)
    sem = _run(c.views, c.output, device, order == "before", DTYPES[dt])
    lab = _run(c.views, c.output, device, order == "before", DTYPES[dt], labels=True)
    assert sem.is_cuda and lab.is_cuda and tuple(sem.shape) == (c.K, *c.output) and tuple(lab.shape) == c.output
    tu.check(sem, lab, e, f"tta {order} {dt}")


@functools.lru_cache(maxsize=None)
def _edge_case(K, Q, order):
    views = tu.synthetic_views(K, Q, seed=K * 1000 + Q)
    return views, tu.expected_from_cpu(views, tu.load().output, order == "before")


@pytest.mark.parametrize("order", tu.ORDERS)
@pytest.mark.parametrize("Q", [32, 100])
@pytest.mark.parametrize("K", [1, 33, 150])
def test_class_and_query_edges(K, Q, order, device):
    """One class, one class past a 32-tile, ADE20K's 150 (five tiles); a whole chunk and three chunks plus a part."""
    views, e = _edge_case(K, Q, order)
    out = tu.load().output
    tu.check(_run(views, out, device, order == "before"), _run(views, out, device, order == "before", labels=True), e,
             f"tta K={K} Q={Q} {order}")


@pytest.mark.parametrize("order", tu.ORDERS)
def test_single_view_agrees_with_fused_head(order, device):
    """V = 1, not mirrored: the existing semantic kernel (plus torch's resize of its scores in the `after` order)."""
    from bm2f_amd import MaskFormerInference
    c = tu.load()
    v = c.views[2]
    before = order == "before"
    m = MaskFormerInference(num_classes=c.K, sem_seg_postprocess_before_inference=before)
    want = m({"pred_logits": v["cls"][None].to(device), "pred_masks": v["masks"][None].to(device)}, v["padded"],
             [v["image"]], [c.output])[0]["sem_seg"]
    iu.check_continuous(_run([v], c.output, device, before), want.cpu().numpy(), f"single view {order}")
    # and at identity geometry (no second stage in either order)
    want = m({"pred_logits": v["cls"][None].to(device), "pred_masks": v["masks"][None].to(device)}, v["padded"],
             [v["image"]])[0]["sem_seg"]
    iu.check_continuous(_run([v], v["image"], device, before), want.cpu().numpy(), f"single view {order}, one stage")


@pytest.mark.parametrize("order", tu.ORDERS)
def test_flip_symmetry(order, device):
    """Wc == Wp and output == image size: bilinear resizing commutes with mirroring, so a mirrored view fed the
    mirrored logits is the plain view of the original logits.  Pins the Wo - 1 - x column independently of the
    fixture (odd width, two column tiles, the second partial)."""
    geometry = [(10, 14, (40, 53), (37, 53), False)]
    (v,) = tu.synthetic_views(19, 20, seed=3, geometry=geometry)
    mirrored = dict(v, masks=v["masks"].flip(-1).contiguous(), flipped=True)
    before = order == "before"
    plain = _run([v], (37, 53), device, before)
    iu.check_continuous(_run([mirrored], (37, 53), device, before), plain.cpu().numpy(), f"flip symmetry {order}")
    # not vacuous: the logits are not mirror-symmetric, so ignoring the flag misses the bar
    wrong = _run([dict(mirrored, flipped=False)], (37, 53), device, before)
    assert (wrong - plain).abs().max() > 2 * iu.RTOL * plain.abs().max()
    # and through the second stage (output != image size), against the CPU path
    e = tu.expected_from_cpu([v, mirrored], (29, 41), before)
    tu.check(_run([v, mirrored], (29, 41), device, before), _run([v, mirrored], (29, 41), device, before, labels=True),
             e, f"flip two-stage {order}")


@pytest.mark.parametrize("order", tu.ORDERS)
def test_window_fallback(order, device):
    """64 x 64 logits onto a 16 x 16 output: a tile's source window (about 14 x 62 texels) exceeds the LDS window
    cap of 176, so the kernel reads the taps from global memory; plain and mirrored."""
    geometry = [(64, 64, (64, 64), (64, 64), False), (64, 64, (64, 64), (60, 62), True)]
    views = tu.synthetic_views(19, 20, seed=5, geometry=geometry)
    before = order == "before"
    e = tu.expected_from_cpu(views, (16, 16), before)
    tu.check(_run(views, (16, 16), device, before), _run(views, (16, 16), device, before, labels=True), e,
             f"window fallback {order}")


def test_deterministic(device):
    c = tu.load()
    for before in (True, False):
        a, b = (_run(c.views, c.output, device, before) for _ in range(2))
        assert torch.equal(a, b)
        a, b = (_run(c.views, c.output, device, before, labels=True) for _ in range(2))
        assert torch.equal(a, b)


def test_labels_mode_allocates_no_score_tensor(device):
    """K = 150, 256 x 320, V = 4: the peak over the call stays below one (K, Ho, Wo) fp32 tensor (49 MB); labels, probs,
    the flat logits and the table are well under 2 MB."""
    K, Q, out = 150, 32, (256, 320)
    geometry = [(32, 40, (128, 160), (128, 160), False), (32, 40, (128, 160), (128, 160), True),
                (48, 64, (192, 256), (192, 240), False), (48, 64, (192, 256), (192, 240), True)]
    views = tu.api_views(tu.synthetic_views(K, Q, seed=9, geometry=geometry), device)
    from bm2f_amd import semantic_inference_tta
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lab = semantic_inference_tta(views, out, num_classes=K, labels=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"labels mode: peak {peak} bytes over the call, one score tensor {K * out[0] * out[1] * 4}")
    assert peak < K * out[0] * out[1] * 4
    assert lab.dtype == torch.int16 and tuple(lab.shape) == out
    sem = semantic_inference_tta(views, out, num_classes=K)
    assert torch.equal(sem.argmax(0).to(torch.int16), lab)     # the same accumulators, the same first maximum


def test_driver_end_to_end(device):
    """The default mapper on a device image and a stub model that returns device tensors."""
    from bm2f_amd import SemanticSegmentorWithTTA, semantic_inference_tta
    K, Q = 19, 20
    g = torch.Generator().manual_seed(1)
    cls = torch.randn(Q, K + 1, generator=g).to(device)
    scale = torch.linspace(-3, 3, Q, device=device).view(1, Q, 1, 1)
    record = []

    def model(batch):
        (x,) = batch
        h, w = x["image"].shape[-2:]
        assert x["image"].is_cuda
        hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
        masks = F.interpolate(x["image"][None, :1].expand(1, Q, h, w) * scale, size=(hp // 4, wp // 4),
                              mode="bilinear", align_corners=False)
        record.append(({"pred_logits": cls, "pred_masks": masks[0]}, (hp, wp), (h, w)))
        return {"pred_logits": cls[None], "pred_masks": masks}, (hp, wp), [(h, w)]

    image = torch.rand(3, 37, 53, generator=g).to(device)
    seg = SemanticSegmentorWithTTA(model, num_classes=K, min_sizes=(40, 75), max_size=200, flip=True)
    out = seg([{"image": image}])
    assert set(out[0]) == {"sem_seg"} and out[0]["sem_seg"].is_cuda and tuple(out[0]["sem_seg"].shape) == (K, 37, 53)
    assert len(record) == 4
    views = [(*r, bool(i % 2)) for i, r in enumerate(record)]
    assert torch.equal(out[0]["sem_seg"], semantic_inference_tta(views, (37, 53), num_classes=K))
    cpu = [({k: t.cpu() for k, t in o.items()}, p, s, f) for o, p, s, f in views]
    iu.check_continuous(out[0]["sem_seg"], semantic_inference_tta(cpu, (37, 53), num_classes=K).numpy(), "driver")
    taller = seg([{"image": image, "height": 50, "width": 70}])[0]["sem_seg"]
    assert tuple(taller.shape) == (K, 50, 70)
