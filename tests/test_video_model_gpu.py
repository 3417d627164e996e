"""Video inference and clip target preparation on the GPU (csrc/video_inference.hip: m2f_infer_video,
m2f_feat_resize_pad): the assertions of test_video_model_cpu.py on the HIP path, plus the kernel's two paths, the
store tails, 16-bit logits, peak memory, the feature resize at a non-integer ratio, and the prepared targets through
the criterion.  Bars: test_video_model_cpu.py; the rest are stated per test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_video_model_cpu as vm
from bm2f_amd import (VideoMaskFormerInference, _native, feat_resize_pad, pack_mask_bits, prepare_video_targets,
                      prepare_video_weaksup_targets)
from bm2f_amd import weaksup

pytestmark = pytest.mark.gpu
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _same(a, b):
    assert a["pred_scores"] == b["pred_scores"] and a["pred_labels"] == b["pred_labels"]
    assert len(a["pred_masks"]) == len(b["pred_masks"]) > 0
    for x, y in zip(a["pred_masks"], b["pred_masks"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", vm.CASES)
def test_inference_vs_reference(name, device):
    m, out, padded, image, output = vm.infer_case(name, device)
    res = m(out, padded, image, output)
    vm.check_inference(res, name)
    vm.check_packed(m(out, padded, image, output, packed=True), res, output[1])


@pytest.mark.parametrize("name", ["d", "a"])
def test_lds_and_direct_paths_agree(name, device):
    """infer_video_cap = 0 sends every tile down the direct path, 4096 texels hold case d's whole 40 x 56 source."""
    m, out, padded, image, output = vm.infer_case(name, device)
    runs = {}
    for cap in (0, 4096):
        with _native.options(infer_video_cap=cap):
            runs[cap] = (m(out, padded, image, output), m(out, padded, image, output, packed=True))
    _same(runs[0][0], runs[4096][0])
    _same(runs[0][1], runs[4096][1])
    vm.check_inference(runs[0][0], name)
    _same(m(out, padded, image, output), runs[0][0])                      # and the default budget


@pytest.mark.parametrize("width", [31, 32, 33, 65])
def test_edge_widths(width, device):
    """Word and tile tails of the byte and the packed stores (a tile is 16 x 64 pixels, a packed word 32): against
    the CPU path outside an fp64 ambiguity map built as the fixture's."""
    m, out, padded, image, _ = vm.infer_case("a", device)
    output = (23, width)
    cpu = {k: v.cpu() for k, v in out.items()}
    want = m(cpu, padded, image, output)
    got = m(out, padded, image, output)
    # topk(sorted=False) fixes no order: entries are paired by (label, score), as against the fixture
    og, ow = vm._order(got["pred_labels"], got["pred_scores"]), vm._order(want["pred_labels"], want["pred_scores"])
    assert np.array_equal(np.asarray(got["pred_labels"])[og], np.asarray(want["pred_labels"])[ow])
    np.testing.assert_allclose(np.asarray(got["pred_scores"])[og], np.asarray(want["pred_scores"])[ow], rtol=1e-6)
    scores = F.softmax(cpu["pred_logits"][0].float(), -1)[:, :-1].flatten()
    qidx = scores.topk(10, sorted=False).indices // m.num_classes
    x = F.interpolate(cpu["pred_masks"][0].double()[qidx], size=padded, mode="bilinear", align_corners=False)
    x = F.interpolate(x[..., :image[0], :image[1]], size=output, mode="bilinear", align_corners=False)
    amb = x.abs() < 1e-5 * x.abs().flatten(1).amax(1).view(-1, 1, 1, 1)
    assert amb.float().mean() <= 0.005
    for i, j in zip(og, ow):                             # amb follows the CPU path's entry order
        g, w = got["pred_masks"][i], want["pred_masks"][j]
        assert tuple(g.shape) == (3, 23, width) and not ((g != w) & ~amb[j]).any()
    vm.check_packed(m(out, padded, image, output, packed=True), got, width)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["a", "d"])
def test_16bit_logits(name, dt, device):
    """16-bit logits are converted on load: the result is the fp32 path's on logits.float(), bit for bit."""
    m, out, padded, image, output = vm.infer_case(name, device)
    g = torch.Generator().manual_seed(1)
    low = (torch.randn(out["pred_masks"].shape, generator=g) * 3).to(DTYPES[dt]).to(device)
    a = m({"pred_logits": out["pred_logits"], "pred_masks": low}, padded, image, output)
    b = m({"pred_logits": out["pred_logits"], "pred_masks": low.float()}, padded, image, output)
    _same(a, b)
    assert any(x.any() for x in a["pred_masks"]) and not all(x.all() for x in a["pred_masks"])


def test_peak_memory(device):
    """Q = 16, T = 4, logits 16 x 24, padded 64 x 96: the call allocates less than half of the (Q, T, Hp, Wp) fp32
    tensor the reference builds (the bool output of 10 masks is 6 % of it)."""
    Q, T, K = 16, 4, 5
    g = torch.Generator().manual_seed(0)
    out = {"pred_logits": torch.randn(1, Q, K + 1, generator=g).to(device),
           "pred_masks": (torch.randn(1, Q, T, 16, 24, generator=g) * 3).to(device)}
    m = VideoMaskFormerInference(K)
    m(out, (64, 96), (64, 96))                          # warm-up: library and kernel load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = m(out, (64, 96), (64, 96))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    reference = Q * T * 64 * 96 * 4
    print(f"peak {peak} bytes over the call; the reference's upsampled tensor {reference} bytes")
    assert len(res["pred_masks"]) == 10 and tuple(res["pred_masks"][0].shape) == (T, 64, 96)
    assert peak < reference // 2


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_feat_resize_non_integer_ratio(dt, device):
    """Source 37 x 45 inside pad 48 x 56 -> 11 x 13: within 1e-6 of max |feature| of fp64 F.interpolate on the
    zero-padded tensor (four products and three sums of fp32 rounding stay under 5e-7)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 5, 37, 45, generator=g).to(dt)
    want = F.interpolate(F.pad(x.double(), (0, 56 - 45, 0, 48 - 37)), size=(11, 13), mode="bilinear",
                         align_corners=False)
    got = feat_resize_pad(x.to(device), (48, 56), (11, 13))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 5, 11, 13)
    err = (got.cpu().double() - want).abs().max().item()
    print(f"max |err| {err:.3e}, max |feature| {x.abs().max().item():.3f}")
    assert err <= 1e-6 * x.double().abs().max().item()


def test_feat_resize_bitwise_on_fixture(device):
    z = vm.gold()
    _, _, feats = vm.clip_inputs(device)
    for b, f in enumerate(feats):
        f = f if torch.is_tensor(f) else torch.cat(f)
        assert np.array_equal(feat_resize_pad(f, (64, 64), (16, 16)).cpu().numpy(), z[f"feats_ds{b}"])
        assert np.array_equal(feat_resize_pad(f.half(), (64, 64), (16, 16)).cpu().numpy(), z[f"feats_ds{b}"])


@pytest.mark.parametrize("as_instances", [False, True], ids=["dicts", "instances"])
def test_weaksup_targets_vs_reference(as_instances, device):
    targets, images, feats = vm.clip_inputs(device, as_instances=as_instances)
    out = prepare_video_weaksup_targets(targets, images, feats, num_frames=3)
    vm.check_targets(out, device)
    assert all(t[k].is_cuda for t in out for k in ("labels", "ids", "box_masks", "masks", "color_similarities"))


def test_lab_vs_reference(device):
    _, images, _ = vm.clip_inputs(device)
    lab = weaksup.images_lab(vm.padded_images(images, device), 4).cpu()
    torch.testing.assert_close(lab, torch.from_numpy(vm.gold()["lab"]), rtol=1e-6, atol=1e-5)


def test_video_targets_on_device(device):
    z = vm.gold()
    targets, _, _ = vm.clip_inputs(device)
    for b, t in enumerate(prepare_video_targets(targets, (64, 64), 3)):
        assert t["masks"].is_cuda and np.array_equal(t["masks"].cpu().numpy(), vm._unpack(z[f"full_masks{b}"], 64))
        assert np.array_equal(t["ids"].cpu().numpy(), z[f"ids{b}"])


def test_targets_through_the_criterion(device, monkeypatch):
    """The prepared targets go into VideoSetCriterionProjSpatPairTempPair as they are: every loss is finite and the
    temporal loss counts as many live pairs as were mined (Q exceeds every clip's targets: all are matched)."""
    from bm2f_amd import VideoHungarianMatcherProjPair, VideoSetCriterionProjSpatPairTempPair
    targets, images, feats = vm.clip_inputs(device)
    tg = prepare_video_weaksup_targets(targets, images, feats, num_frames=3)
    mined = sum(int(t["total_temp_pair"]) for t in tg)
    assert mined > 0
    B, Q, K, T = len(tg), 8, 5, 3
    w = {"loss_ce": 2.0, "loss_mask_projection": 5.0, "loss_mask_spatial_pairwise": 5.0,
         "loss_mask_temporal_pairwise": 3.0}
    matcher = VideoHungarianMatcherProjPair(cost_class=2.0, cost_projection=5.0, cost_pairwise=5.0,
                                            pairwise_warmup_iters=2)
    crit = VideoSetCriterionProjSpatPairTempPair(
        K, matcher=matcher, weight_dict=w, eos_coef=0.1, pairwise_size=3, pairwise_dilation=2,
        pairwise_color_thresh=0.3, pairwise_warmup_iters=2,
        losses=["labels", "projection_masks", "spatial_pairwise", "temporal_pairwise"]).to(device)
    counts = []
    pair_sum = weaksup.temporal_pair_sum

    def spy(src, row_of_target, pk):
        total, count = pair_sum(src, row_of_target, pk)
        counts.append(count)
        return total, count

    monkeypatch.setattr(weaksup, "temporal_pair_sum", spy)
    g = torch.Generator().manual_seed(9)
    for _ in range(2):                                   # the second call has a non-zero warm-up factor
        out = {"pred_logits": torch.randn(B, Q, K + 1, generator=g).to(device).requires_grad_(),
               "pred_masks": (torch.randn(B, Q, T, 16, 16, generator=g) * 3).to(device).requires_grad_()}
        losses = crit(out, tg)
        assert set(losses) == set(w)
        assert all(torch.isfinite(v).all() for v in losses.values())
        sum(v.sum() * w[k] for k, v in losses.items()).backward()
        assert torch.isfinite(out["pred_masks"].grad).all()
    assert len(counts) == 2 and all(int(c) == mined for c in counts)
    assert float(losses["loss_mask_temporal_pairwise"].detach()) > 0
