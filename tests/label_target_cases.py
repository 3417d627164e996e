"""Shared checks of the label-map training targets (bm2f_amd/label_targets.py and the label-map paths of
bm2f_amd/mask_criterion.py), run on the CPU by test_label_targets_cpu.py and on the device by
test_label_targets_gpu.py.

Oracles: the project's own dense path (held to the reference's fixture by test_mask_criterion_*.py) given
``label_targets_to_masks`` of the same targets, and a restatement of the two reference mappers' target construction
(``np.unique`` / ``==``) below."""
import numpy as np
import pytest
import torch

from bm2f_amd import (HungarianMatcher, SetCriterion, VideoHungarianMatcher, VideoSetCriterion, label_histogram_ragged,
                      label_targets_to_masks, panoptic_targets, semantic_targets)
from bm2f_amd import label_counts
from test_mask_criterion_cpu import pool_source

MAP_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)
IGNORE = 255


# ------------------------------------------------------------------------------------------------------------
# the reference mappers' target construction, restated
# ------------------------------------------------------------------------------------------------------------
def mapper_semantic(sem_seg, ignore_label):
    """MaskFormerSemanticDatasetMapper: classes = np.unique(sem_seg) without ignore; masks = [sem_seg == c]."""
    classes = np.unique(sem_seg)
    classes = classes[classes != ignore_label]
    return classes.astype(np.int64), [sem_seg == c for c in classes]


def mapper_panoptic(pan_seg, segments_info):
    """MaskFormerPanopticDatasetMapper: one (category_id, pan_seg == id) per non-crowd segment, in list order."""
    classes, masks = [], []
    for s in segments_info:
        if not s["iscrowd"]:
            classes.append(s["category_id"])
            masks.append(pan_seg == s["id"])
    return np.array(classes, dtype=np.int64), masks


def blocky(g, h, w, values, cell=4):
    """(h, w) int64 map of piecewise-constant regions with values drawn from `values`."""
    gh, gw = -(-h // cell), -(-w // cell)
    pick = torch.randint(len(values), (gh, gw), generator=g)
    coarse = torch.as_tensor(values, dtype=torch.int64)[pick]
    return coarse.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:h, :w].contiguous()


def _check_target(t, classes, masks, ids, device, shape):
    assert t["labels"].dtype == torch.int64 and t["labels"].device.type == device.type
    assert t["ids"].device.type == device.type and t["label_map"].device.type == device.type
    assert t["labels"].cpu().tolist() == classes.tolist()
    assert t["ids"].cpu().tolist() == list(ids)
    dense = label_targets_to_masks(t)
    assert dense.dtype == torch.bool and tuple(dense.shape) == (len(classes), *shape)
    want = np.stack(masks) if masks else np.zeros((0, *shape), bool)
    assert np.array_equal(dense.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------
def check_semantic_targets(device, dtype):
    g = torch.Generator().manual_seed(11)
    num_classes = 150 if dtype != torch.uint8 else 19
    present = [[3, 0, 17, IGNORE], [IGNORE], [num_classes - 1, 5, 6, 7, 8, 2], [4]]
    sizes = [(37, 53), (16, 24), (64, 41), (9, 7)]                     # different sizes, none a multiple of 8 wide
    segs = [blocky(g, h, w, v).to(dtype) for (h, w), v in zip(sizes, present)]
    out = semantic_targets([s.to(device) for s in segs], IGNORE, num_classes)
    assert len(out) == len(segs)
    for t, s, size in zip(out, segs, sizes):
        classes, masks = mapper_semantic(s.numpy().astype(np.int64), IGNORE)
        _check_target(t, classes, masks, classes.tolist(), device, size)
        assert t["areas"].cpu().tolist() == [int(m.sum()) for m in masks]
        assert t["label_map"].dtype == (dtype if dtype != torch.int64 else torch.int32)
    assert out[1]["labels"].numel() == 0                                # the all-ignored image
    # a value that is neither a class nor the ignore label: ValueError naming the image
    bad = [s.clone() for s in segs]
    bad[2][5, 6] = num_classes
    with pytest.raises(ValueError, match="image 2"):
        semantic_targets([s.to(device) for s in bad], IGNORE, num_classes)


def check_panoptic_targets(device, dtype):
    g = torch.Generator().manual_seed(12)
    top = 2 ** 24 - 1
    if dtype == torch.uint8:
        idsets = [[1, 2, 200, 0], [7, 0], [9, 10, 11, 0]]
    elif dtype == torch.int16:
        idsets = [[1, 2, 30000, 0], [7, 0], [9, 10, 11, 0]]
    else:
        idsets = [[top, top - 1, 2 ** 23, 0], [7, 0], [top - 256, 10, 11, 0]]           # ids near 2^24; 0 is VOID
    sizes = [(37, 53), (16, 24), (64, 41)]
    pans = [blocky(g, h, w, v).to(dtype) for (h, w), v in zip(sizes, idsets)]
    absent = 123 if dtype == torch.uint8 else 12345
    infos = []
    for b, v in enumerate(idsets):
        segs = [{"id": i, "category_id": 3 * k + b, "iscrowd": 0} for k, i in enumerate(v[:-1])]
        segs = segs[::-1]                                               # list order, not id order
        if b == 0:
            segs[1]["iscrowd"] = 1                                      # a crowd segment is dropped
            segs.insert(1, {"id": absent, "category_id": 77, "iscrowd": 0})   # listed, no pixels: kept, empty
        infos.append(segs)
    out = panoptic_targets([p.to(device) for p in pans], infos)
    for t, p, segs, size in zip(out, pans, infos, sizes):
        classes, masks = mapper_panoptic(p.numpy().astype(np.int64), segs)
        _check_target(t, classes, masks, [s["id"] for s in segs if not s["iscrowd"]], device, size)
        if device.type == "cuda":
            assert t["ids"].dtype == torch.int32
    dense0 = label_targets_to_masks(out[0])
    assert dense0.shape[0] == 3 and not dense0[1].any() and dense0[0].any() and dense0[2].any()
    # an image without segments
    none = panoptic_targets([pans[0].to(device)], [[]])
    assert none[0]["labels"].numel() == 0 and label_targets_to_masks(none[0]).shape == (0, *sizes[0])


def check_histogram(device, dtype, bins):
    """label_histogram_ragged against np.bincount, exact: plane sizes that are no multiple of the vector width, an
    empty plane and a plane that is an offset view of a larger buffer."""
    g = torch.Generator().manual_seed(bins)
    top = min(bins, 250 if dtype == torch.uint8 else 30000 if dtype == torch.int16 else bins)
    ignore = 255 if dtype == torch.uint8 else -1
    sizes = [(37, 53), (0, 5), (129, 67), (3, 3), (1, 8191)]
    planes = []
    for h, w in sizes:
        p = torch.randint(top, (h, w), generator=g)
        p[torch.rand(h, w, generator=g) < 0.1] = ignore
        if h * w > 100:                                                 # long runs of one value, as label maps have
            p.view(-1)[10:90] = top - 1
        planes.append(p.to(dtype))
    big = torch.zeros(5 + 41 * 23 + 3, dtype=dtype)
    view = big[5:5 + 41 * 23].view(41, 23)                             # starts 5 elements into its storage
    view.copy_(torch.randint(top, (41, 23), generator=g).to(dtype))
    on_dev = [p.to(device) for p in planes] + [big.to(device)[5:5 + 41 * 23].view(41, 23)]
    host = [p.numpy() for p in planes] + [view.numpy()]
    paths = ["auto"]
    if device.type == "cuda":
        assert on_dev[-1].storage_offset() == 5
        paths.append("global")
        if bins + 1 <= label_counts.geometry()[2]:
            paths.append("lds")
    for path in paths:
        counts, bad = label_histogram_ragged(on_dev, bins, ignore, path=path)
        assert counts.shape == (len(host), bins + 1) and counts.dtype == np.int64
        for i, p in enumerate(host):
            a = p.reshape(-1).astype(np.int64)
            want = np.bincount(a[a != ignore], minlength=bins)
            assert np.array_equal(counts[i, :bins], want), (path, i)
            assert counts[i, bins] == int((a == ignore).sum()) and bad[i] == 0
    # without an ignore label the ignored pixels are bad (uint8) or negative (bad as well)
    counts, bad = label_histogram_ragged(on_dev[:1], bins)
    a = host[0].reshape(-1).astype(np.int64)
    assert bad[0] == int(((a < 0) | (a >= bins)).sum()) and counts[0, bins] == 0
    assert np.array_equal(counts[0, :bins], np.bincount(a[(a >= 0) & (a < bins)], minlength=bins))


# ------------------------------------------------------------------------------------------------------------
# whole criterion and matcher
# ------------------------------------------------------------------------------------------------------------
NUM_CLASSES = 12
SIZES = [(40, 52), (36, 44), (48, 40)]


def criterion_case(map_dtype=torch.int32):
    """Three images of different sizes as panoptic label maps (one listed segment without pixels, VOID pixels) and
    three heads of predictions (B, Q = 10, 12, 14)."""
    g = torch.Generator().manual_seed(5)
    idsets = [[10, 20, 30, 40, 0], [5, 0], [7, 8, 9, 0]]
    pans = [blocky(g, h, w, v, cell=8).to(map_dtype) for (h, w), v in zip(SIZES, idsets)]
    infos = [[{"id": i, "category_id": (i + b) % NUM_CLASSES, "iscrowd": 0} for i in v[:-1]]
             for b, v in enumerate(idsets)]
    infos[2].append({"id": 99, "category_id": 1, "iscrowd": 0})                       # no pixels
    heads = [{"pred_logits": torch.randn(3, 10, NUM_CLASSES + 1, generator=g),
              "pred_masks": torch.randn(3, 10, 12, 14, generator=g) * 3} for _ in range(3)]
    return pans, infos, heads


def build(video=False, num_points=50):
    matcher = (VideoHungarianMatcher if video else HungarianMatcher)(cost_class=2.0, cost_mask=5.0, cost_dice=5.0,
                                                                     num_points=num_points)
    crit = (VideoSetCriterion if video else SetCriterion)(
        NUM_CLASSES, matcher=matcher, weight_dict={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}, eos_coef=0.1,
        losses=["labels", "masks"], num_points=num_points, oversample_ratio=3.0, importance_sample_ratio=0.75)
    crit.point_source = pool_source()
    return matcher, crit


def run_criterion(device, targets, heads, keep=slice(None), mask_dtype=torch.float32):
    matcher, crit = build()
    crit = crit.to(device)
    seen = []
    orig = matcher.memory_efficient_forward

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(r)
        return r

    matcher.memory_efficient_forward = spy
    hs = [{"pred_logits": h["pred_logits"][keep].to(device).requires_grad_(),
           "pred_masks": h["pred_masks"][keep].to(device=device, dtype=mask_dtype).requires_grad_()} for h in heads]
    losses = crit(dict(hs[-1], aux_outputs=hs[:-1]), targets)
    sum(v.sum() for v in losses.values()).backward()
    return losses, seen, hs


def to_dense(targets):
    return [{"labels": t["labels"], "masks": label_targets_to_masks(t)} for t in targets]


def same_loss(key, got, want, bitwise):
    """CPU: rtol 1e-5.  Device: the mask losses, which are what reads the targets, are bitwise equal.  ``loss_ce`` reads
    no mask target: with identical indices (asserted by the callers) both runs hand torch's weighted
    ``F.cross_entropy`` identical inputs, but on the device that op adds its per-image partial sums with float atomics
    and two identical calls differ in the last bits.  It is held to the reordering bound of an fp32 sum of the B Q = 30
    terms, 30 * 2^-24 < 2e-6 relative."""
    a, b = float(got.detach()), float(want.detach())
    if not bitwise:
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=0, err_msg=key)
    elif key.startswith("loss_ce"):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=0, err_msg=key)
    else:
        assert torch.equal(got.detach(), want.detach()), key


def check_criterion(device, bitwise, map_dtype=torch.int32, mask_dtype=torch.float32):
    """Label-map targets against their dense equivalents through SetCriterion with three heads and a fixed point
    source: indices identical, losses bitwise equal (device) or within rtol 1e-5 (CPU), gradients within rtol 1e-4 /
    atol 1e-6 (fp16 masks: 2^-10, the rounding of the gradient to fp16)."""
    pans, infos, heads = criterion_case(map_dtype)
    targets = panoptic_targets([p.to(device) for p in pans], infos)
    got, idx_l, hs_l = run_criterion(device, targets, heads, mask_dtype=mask_dtype)
    want, idx_d, hs_d = run_criterion(device, to_dense(targets), heads, mask_dtype=mask_dtype)
    assert len(idx_l) == len(idx_d) == 3
    for a, b in zip(idx_l, idx_d):
        for (i0, j0), (i1, j1) in zip(a, b):
            assert torch.equal(i0, i1) and torch.equal(j0, j1)
    assert [len(i) for i, _ in idx_l[0]] == [4, 1, 4]
    assert sorted(got) == sorted(want) and len(got) == 9
    for k in want:
        print(f"{k}: label {float(got[k].detach()):.9g} dense {float(want[k].detach()):.9g}")
        assert float(got[k].detach()) > 0
        same_loss(k, got[k], want[k], bitwise)
    rtol = 1e-4 if mask_dtype == torch.float32 else 2.0 ** -10
    for a, b in zip(hs_l, hs_d):
        for k in a:
            assert a[k].grad.dtype == a[k].dtype and a[k].grad.any()
            np.testing.assert_allclose(a[k].grad.float().cpu().numpy(), b[k].grad.float().cpu().numpy(),
                                       rtol=rtol if k == "pred_masks" else 1e-4, atol=1e-6, err_msg=k)


def check_empty_and_errors(device, bitwise):
    pans, infos, heads = criterion_case()
    maps = [p.to(device) for p in pans]
    # no targets at all: zero mask losses, still connected to pred_masks
    none = panoptic_targets(maps, [[] for _ in infos])
    out, _, hs = run_criterion(device, none, heads)
    for k, v in out.items():
        if not k.startswith("loss_ce"):
            assert float(v.detach()) == 0.0, k
    for h in hs:
        assert h["pred_masks"].grad is not None and not h["pred_masks"].grad.any()
    # one image with G = 0 (the last): what the dense targets give, and no gradient into its masks
    mixed = panoptic_targets(maps, infos[:-1] + [[]])
    got, idx_l, hs = run_criterion(device, mixed, heads)
    want, idx_d, _ = run_criterion(device, to_dense(mixed), heads)
    for a, b in zip(idx_l, idx_d):
        for (i0, j0), (i1, j1) in zip(a, b):
            assert torch.equal(i0, i1) and torch.equal(j0, j1)
    for k in want:
        same_loss(k, got[k], want[k], bitwise)
    for h in hs:
        assert not h["pred_masks"].grad[-1].any() and h["pred_masks"].grad[:-1].any()
    # a batch is all dense or all label maps
    full = panoptic_targets(maps, infos)
    with pytest.raises(ValueError, match="all dense masks or all label maps"):
        run_criterion(device, to_dense(full[:1]) + full[1:], heads)
    both = [dict(t, masks=label_targets_to_masks(t)) for t in full]
    with pytest.raises(ValueError, match="all dense masks or all label maps"):
        run_criterion(device, both, heads)
    # the video classes take dense masks only
    matcher, crit = build(video=True)
    vid = {"pred_logits": heads[0]["pred_logits"].to(device), "pred_masks": heads[0]["pred_masks"][:, :, None].to(device)}
    with pytest.raises(ValueError, match="video"):
        crit.to(device)(vid, full)
    with pytest.raises(ValueError, match="video"):
        matcher(vid, full)
    # mask_target_type="box_mask": the loss keeps reading box_masks_full, the matcher reads the label maps
    boxed = [dict(t, box_masks_full=label_targets_to_masks(t)) for t in full]
    res = []
    for ts in (boxed, [dict(t, box_masks_full=t["masks"]) for t in to_dense(full)]):
        _, crit = build()
        crit.mask_target_type = "box_mask"
        crit = crit.to(device)
        idx = [(torch.arange(t["labels"].shape[0], device=device),) * 2 for t in ts]
        res.append(crit.get_loss("masks", {k: v.to(device) for k, v in heads[0].items()}, ts, idx, 7.0))
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
