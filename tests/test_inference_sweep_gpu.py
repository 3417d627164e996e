"""The fused image inference heads (csrc/inference.hip) over the class, query and size edges of inference_cases.py:
every semantic_kernel<KT>, the global-load path, query chunking up to kMaxQ, tile tails, the strided combine loop,
the selection edges and non-finite logits.  test_inference_sweep_cpu.py asserts that each case reaches its branch.

Every case runs MaskFormerInference with the three heads on, in score mode and in labels mode, plus
panoptic_counters, against the CPU path with fp64 ambiguity maps (``iu.expected_from_cpu``).  Bars:
inference_util.py, unchanged.  K = 1 is the one omission: the fp64 evaluation takes a top-2 over classes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inference_cases as ic
import inference_util as iu

pytestmark = pytest.mark.gpu


def _outputs(c, dt, device, masks=None):
    masks = c.masks if masks is None else masks
    return {"pred_logits": c.cls.to(device), "pred_masks": masks.to(ic.DTYPES[dt]).to(device)}


def _run(c, out, labels=False):
    return iu.module(c)(out, c.padded, c.image_sizes, c.output_sizes, semantic_labels=labels)


def _counters(c, out):
    from bm2f_amd.inference import panoptic_counters
    return panoptic_counters(out["pred_logits"], out["pred_masks"], c.padded, c.image_sizes, c.output_sizes,
                             num_classes=c.K, object_mask_threshold=c.thresholds[0])


def _sweep(name, dt, device):
    """The common procedure; returns the score-mode results."""
    c, exp = ic.get(name), ic.expected(name, dt)
    out = _outputs(c, dt, device)
    res = _run(c, out)
    iu.check_results(res, c, exp)
    iu.check_results(_run(c, out, labels=True), c, exp, labels=True)
    for b, got in enumerate(_counters(c, out)):
        iu.check_counters(got, exp[b], f"{name}{b} counters")
    return res


@pytest.mark.parametrize("k", ic.K_SWEEP)
def test_classes(k, device):
    """semantic_kernel<ceil(K / 32)>: zero padding at K = 32 n and 32 n + 1, the 79 KB LDS request at KT = 8, and
    the epilogue's class index map -- on ``cls_ramp`` every class plane differs from every other by more than the
    bar, so a class written to the wrong plane fails."""
    c = ic.get(f"K{k}")
    _sweep(c.name, "fp32", device)
    m = iu.module(c, instance_on=False, panoptic_on=False, sem_seg_postprocess_before_inference=True)
    out = {"pred_logits": c.cls_ramp.to(device), "pred_masks": c.masks.to(device)}
    got = m(out, c.padded, c.image_sizes, c.output_sizes)
    for b, want in enumerate(ic.ramp_expected(c)):
        iu.check_continuous(got[b]["sem_seg"], want.numpy(), f"{c.name}{b} ramp sem_seg")


@pytest.mark.parametrize("q", ic.Q_SWEEP)
def test_queries(q, device):
    """Chunks of kQC = 32 queries: 1, 31, 32, 33, ... up to kMaxQ = 256 with every query kept (nk == Q)."""
    _sweep(f"Q{q}", "fp32", device)


@pytest.mark.parametrize("dt", list(ic.DTYPES))
@pytest.mark.parametrize("name", ic.SIXTEEN_BIT)
def test_direct_path_and_dtypes(name, dt, device):
    """Downscaling tiles read global memory (window > kWinCap); the mixed batches take both paths in one launch and
    have an image smaller than the output buffer.  16-bit logits: the CPU path on ``masks.float()``."""
    _sweep(name, dt, device)


@pytest.mark.parametrize("name", ic.TAILS)
def test_tails(name, device):
    """Semantic 4 x 32, panoptic 4 x 64 and instance 1024-pixel tile tails; 1 x 7, 7 x 1 and 2 x 2 sources (the
    i1 = i0 + (i0 < in - 1) clamp); topk == Q * K."""
    _sweep(name, "fp32", device)


def test_many_tiles(device):
    """67 instance tiles: instance_combine_kernel's lanes 0..2 add two partials each.  Beyond the common bars, the
    scores are held to an fp64 recomputation from the full-resolution logits, and the kernel's own sums to its own
    masks: the pixel count exactly (integers below 2^24 in fp32), the sigmoid sum within 1e-5 relative (fp32
    rounding of about 34 000 terms added in a tree stays below 1e-6; one lost tile is 1.5e-2)."""
    from bm2f_amd import _native
    c = ic.get("many_tiles")
    assert ic.instance_tiles(c) == 67
    res = _sweep("many_tiles", "fp32", device)
    full = ic.full64(c, 0)
    on = full > 0
    mask_score = (full.sigmoid() * on).flatten(1).sum(1) / (on.flatten(1).sum(1) + 1e-6)
    table = F.softmax(c.cls[0].double(), -1)[:, :c.things] * mask_score[:, None]          # (Q, things)
    want_cls = torch.arange(c.things).expand(c.Q, -1).flatten().numpy()
    want, got = table.flatten().numpy(), res[0]["instances"]
    gs, gc = got["scores"].cpu().numpy(), got["pred_classes"].cpu().numpy()
    og, ow = np.lexsort((gs, gc)), np.lexsort((want, want_cls))
    assert np.array_equal(gc[og], want_cls[ow])
    iu.check_continuous(gs[og], want[ow], "many_tiles scores vs fp64")

    (h, w), (Hp, Wp), (Ho, Wo), Q = c.masks.shape[-2:], c.padded, c.output_sizes[0], c.Q
    tiles = ic.instance_tiles(c)
    masks = c.masks.to(device)
    sizes = torch.tensor([[*c.image_sizes[0], Ho, Wo]], dtype=torch.int32, device=device)
    sel = torch.arange(Q, dtype=torch.int32, device=device)
    n_sel = torch.tensor([Q], dtype=torch.int32, device=device)
    binary = torch.empty((1, Q, Ho, Wo), dtype=torch.uint8, device=device)
    partials = torch.full((1, Q, tiles, 2), float("nan"), device=device)
    sums = torch.empty((1, Q, 2), device=device)
    _native.call("m2f_infer_instance", masks.data_ptr(), 0, sel.data_ptr(), n_sel.data_ptr(), sizes.data_ptr(), 1, Q,
                 Q, h, w, Hp, Wp, Ho, Wo, tiles, binary.data_ptr(), partials.data_ptr(), sums.data_ptr(),
                 torch.cuda.current_stream(device).cuda_stream)
    own = binary[0].cpu().bool()
    amb = ic.expected("many_tiles")[0].thr_amb
    assert not ((own != on) & ~torch.from_numpy(amb)).any()
    per_tile = F.pad(own.flatten(1), (0, tiles * ic.INSTANCE_TILE - Ho * Wo)).view(Q, tiles, -1).sum(-1)
    assert torch.equal(partials[0, :, :, 1].cpu(), per_tile.float())
    assert torch.equal(sums[0, :, 1].cpu(), own.flatten(1).sum(1).float())
    want_sum = (full.sigmoid() * own).flatten(1).sum(1)
    err = ((sums[0, :, 0].cpu().double() - want_sum).abs() / want_sum).max().item()
    print(f"many_tiles sigmoid sums: max relative error {err:.3e}, bar 1e-5")
    assert (own.flatten(1).sum(1) > 0).all() and err <= 1e-5


def test_none_kept(device):
    res = _sweep("none_kept", "fp32", device)
    pan, info = res[0]["panoptic_seg"]
    assert info == [] and not pan.any()


def test_no_thing_class(device):
    """thing_classes = (): the instance result is empty with the right shapes; the other heads as usual."""
    c, e = ic.get("no_things"), ic.expected("no_things")[0]
    out = _outputs(c, "fp32", device)
    for labels in (False, True):
        r = _run(c, out, labels=labels)[0]
        if labels:
            iu.check_sem_labels(r["sem_seg_labels"], e)
        else:
            iu.check_sem_seg(r["sem_seg"], e)
        iu.check_panoptic(r["panoptic_seg"], e)
        inst = r["instances"]
        assert tuple(inst["pred_masks"].shape) == (0, *c.output_sizes[0]) and inst["pred_masks"].dtype == torch.float32
        assert tuple(inst["scores"].shape) == (0,) and tuple(inst["pred_classes"].shape) == (0,)
        assert tuple(inst["pred_boxes"].shape) == (0, 4) and tuple(inst["image_size"]) == c.output_sizes[0]
    iu.check_counters(_counters(c, out)[0], e)


def test_identical_queries_first_wins(device):
    """Two kept queries with the same logits tie at every pixel: the first maximum wins, as torch.argmax on the CPU
    path.  The fp64 margins flag every such pixel as ambiguous, so the tie is also held directly: the segment list is
    the CPU path's (the second twin winning a pixel would add a segment) and the first twin's segment covers the
    same pixels, except where its own logit is within the threshold margin."""
    c, e = ic.get("twins"), ic.expected("twins")[0]
    res = _sweep("twins", "fp32", device)
    a, _ = ic.twin_queries(c)
    seg = [s["id"] for s in e.segments_info if s["category_id"] == int(c.cls[0, a].argmax())]
    assert len(seg) == 1
    pan, info = res[0]["panoptic_seg"]
    assert info == e.segments_info
    diff = ((pan.cpu().numpy() == seg[0]) != (e.panoptic_seg == seg[0])) & ~e.thr_amb[a]
    others = e.pan_amb & (e.pan_top != seg[0])          # near ties between other queries
    assert (e.panoptic_seg == seg[0]).sum() > 0 and not (diff & ~others).any()


def test_infinite_logits(device):
    """+inf / -inf texels (sigmoid exactly 1 / 0, no NaN): equal to the CPU path under the common bars."""
    c = ic.get("inf")
    assert c.masks.isinf().sum() == 3 and ic.full64(c, 0).isinf().any() and not ic.full64(c, 0).isnan().any()
    _sweep("inf", "fp32", device)


def test_nan_logits(device):
    """The header comment of inference.hip: where every score is NaN the labels map holds -1 and the panoptic winner
    is the first kept query (as torch.argmax on the CPU path, so counters and segments equal the CPU path's); the
    score planes are NaN there; the instance head leaves the pixel out of the mask and of the score.  Every other
    pixel is held to the clean case's expectation."""
    c, masks, reach, cpu, cpu_counters = ic.nan_case()
    e = ic.expected("nan_clean")[0]
    out = _outputs(c, "fp32", device, masks)
    r, rl = _run(c, out)[0], _run(c, out, labels=True)[0]
    sem = r["sem_seg"].cpu().numpy()
    assert np.isnan(sem[:, reach]).all() and not np.isnan(sem[:, ~reach]).any()
    iu.check_sem_seg(np.where(reach, e.sem_seg, sem), e, "nan sem_seg outside")
    lab = rl["sem_seg_labels"]
    assert (lab.cpu().numpy()[reach] == -1).all()
    iu.check_sem_labels(torch.where(torch.from_numpy(reach), torch.from_numpy(e.sem_labels).to(torch.int16), lab.cpu()),
                        e, "nan sem_labels outside")
    for got in (r, rl):
        pan, info = got["panoptic_seg"]
        assert info == cpu["panoptic_seg"][1] == e.segments_info
        assert not pan.cpu().numpy()[reach].any()
        iu.check_discrete(pan, cpu["panoptic_seg"][0].numpy(), e.pan_amb & ~reach,
                          [e.pan_alt, e.pan_top, np.zeros_like(e.pan_alt)], "nan panoptic_seg")
    # counters: the NaN pixels belong to the first kept query, far more of them than ambiguous pixels
    want = SimpleNamespace(**{**vars(e), "counters": cpu_counters})
    assert cpu_counters[0, 0] >= reach.sum() > int(e.pan_amb.sum()) + int(e.thr_amb[e.keep_queries].sum())
    iu.check_counters(_counters(c, out)[0], want, "nan counters")
    inst = r["instances"]
    assert len(inst["scores"]) == len(e.inst_scores) > 0 and torch.isfinite(inst["scores"]).all()
    assert not inst["pred_masks"].cpu().numpy()[:, reach].any()
    part = inst["pred_masks"].flatten(1).mean(1)
    assert ((part > 0) & (part < 1)).any()


@pytest.mark.parametrize("name", ["many_tiles", "Q256"])
def test_two_calls_are_bitwise_identical(name, device):
    """The fixed-order combine over 67 tiles and the integer atomics over 256 kept queries, at their largest."""
    c = ic.get(name)
    out = _outputs(c, "fp32", device)
    a, b = _run(c, out), _run(c, out)
    la, lb = _run(c, out, labels=True), _run(c, out, labels=True)
    ca, cb = _counters(c, out), _counters(c, out)
    assert sum(len(x) for x in ca) > 0
    for x, y in zip(ca, cb):
        assert torch.equal(x, y)
    for ra, rb in zip(la, lb):
        assert torch.equal(ra["sem_seg_labels"], rb["sem_seg_labels"])
    for ra, rb in zip(a, b):
        assert torch.equal(ra["sem_seg"], rb["sem_seg"])
        assert torch.equal(ra["panoptic_seg"][0], rb["panoptic_seg"][0]) and ra["panoptic_seg"][1] == rb["panoptic_seg"][1]
        for k in ("pred_masks", "scores", "pred_classes"):
            assert torch.equal(ra["instances"][k], rb["instances"][k])
