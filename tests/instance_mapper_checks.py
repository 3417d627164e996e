"""The checks of the instance mappers, run on the CPU by test_instance_mappers_cpu.py and on the device by
test_instance_mappers_gpu.py.  The oracle is the dense route of the same commit: every annotation unpacked to a uint8
plane, one ``label_views(seg_pad=0)`` call per image, numpy boxes.  Every comparison is equality."""
import numpy as np
import torch

import instance_view_cases as ivc
from bm2f_amd import instance_mappers as im
from bm2f_amd.image_views import View, label_views
from bm2f_amd.polygon import polygons_to_bits
from bm2f_amd.video_targets import prepare_video_targets, prepare_video_weaksup_targets

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
NUM_CLASSES = 12


def to_rle(mask):
    """Uncompressed COCO RLE of an (H, W) mask: column-major run lengths starting with zeros."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    change = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate(([0], change, [flat.size]))).tolist()
    return {"size": list(mask.shape), "counts": counts if flat[0] == 0 else [0] + counts}


def image(hw, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=hw + (3,), dtype=np.uint8))


def annotations(hw, n, seed, form):
    """n annotations of blobs and noise (one crowd, to be dropped): -> (annotation dicts, the kept dense masks)."""
    kinds = [("blob", "noise", "last", "first")[j % 4] for j in range(n)]
    masks = [ivc.case_masks(hw, (k,), seed=seed + j)[0] for j, k in enumerate(kinds)]
    anns = []
    for j, m in enumerate(masks):
        seg = to_rle(m) if form == "rle" or (form == "mixed" and j % 2 == 0) else (torch.from_numpy(m) if j % 4 == 1
                                                                                  else m.astype(bool))
        anns.append({"segmentation": seg, "category_id": (seed + j) % NUM_CLASSES, "iscrowd": int(j == 2),
                     "id": 10 + j, "keypoints": [0, 0, 0]})
    return anns, [m for j, m in enumerate(masks) if j != 2]


def dense_route(masks, view, device):
    """(G, H, W) uint8 masks under one view by label_views, and numpy boxes: -> (masks (G, Hc, Wc), boxes)."""
    Hc, Wc = ivc.canvas_of(view)
    if len(masks) == 0:
        return torch.zeros((0, Hc, Wc), dtype=torch.uint8, device=device), torch.zeros((0, 4), device=device)
    planes = torch.from_numpy(np.stack(masks)).to(device)
    import dataclasses
    out = label_views([planes], [dataclasses.replace(view, source=0, color=None)], seg_pad=0)[0][0]
    boxes, _ = ivc.bitmask_boxes(out.cpu().numpy())
    return out, torch.from_numpy(boxes).to(device)


def same_instances(got, masks, labels, view, device):
    want_m, want_b = dense_route(masks, view, device)
    assert got["masks"].dtype == torch.uint8 and torch.equal(got["masks"], want_m)
    assert got["boxes"].dtype == torch.float32 and torch.equal(got["boxes"], want_b)
    assert got["labels"].tolist() == labels


def instance_mapper(**kw):
    return im.InstanceTrainMapper(min_sizes=(40, 48), max_size=80, crop_size=(36, 44), num_classes=NUM_CLASSES,
                                  pixel_mean=MEAN, pixel_std=STD, size_divisibility=64, **kw)


SHAPES = [(40, 33), (40, 70), (50, 45)]
COUNTS = [5, 0, 9]


def samples(device, form):
    out, dense = [], []
    for i, (hw, n) in enumerate(zip(SHAPES, COUNTS)):
        anns, masks = annotations(hw, n, 7 * i, form)
        out.append((image(hw, i).to(device), anns))
        dense.append(masks)
    return out, dense


def rle_route_equals_dense(device, form="rle"):
    smp, dense = samples(device, form)
    res = instance_mapper()(smp, np.random.default_rng(3))
    assert res["images"].shape[0] == 3 and res["image_sizes"] == [(64, 64)] * 3
    for i, t in enumerate(res["instances"]):
        labels = [a["category_id"] for a in smp[i][1] if not a["iscrowd"]]
        same_instances(t, dense[i], labels, res["views"][i], device)
    again = instance_mapper()(smp, views=res["views"])                    # a replayed draw
    for a, b in zip(res["instances"], again["instances"]):
        assert all(torch.equal(a[k], b[k]) for k in ("labels", "masks", "boxes"))
    assert torch.equal(res["images"], again["images"])
    bits = instance_mapper(mask_format="bits")(smp, views=res["views"])
    for a, b in zip(res["instances"], bits["instances"]):
        assert np.array_equal(ivc.unpack(b["masks"].cpu().numpy(), 64)[0], a["masks"].cpu().numpy())
    return res, smp


POLYS = [[[4.0, 3.0, 28.5, 6.0, 20.0, 31.0, 6.5, 25.0]], [[10.0, 10.0, 30.0, 10.0, 30.0, 12.0, 10.0, 12.0],
                                                          [2.0, 30.0, 12.0, 30.0, 7.0, 38.5]],
         [[0.0, 0.0, 3.0, 0.0, 0.0, 3.0]]]


def polygon_route(device):
    """Masks equal polygons_to_bits of the host-transformed vertices on the crop window cut by the canvas."""
    hw = (40, 33)
    views = [View(size=(60, 50), crop=(5, 8, 48, 40), canvas=(64, 64), flip_out=True, fill=128),
             View(size=(30, 25), flip_in=True, source=1, fill=128)]
    anns = [{"segmentation": p, "category_id": j} for j, p in enumerate(POLYS)]
    smp = [(image(hw, 0).to(device), anns), (image(hw, 1).to(device), anns[:2])]
    res = instance_mapper()(smp, views=views)
    for i, (v, t) in enumerate(zip(views, res["instances"])):
        n = len(smp[i][1])
        ph, pw = im._plane_size(v, hw)
        moved = [im.transform_polygons(a["segmentation"], v, hw) for a in smp[i][1]]
        planes = ivc.unpack(polygons_to_bits(moved, (ph, pw), device).cpu().numpy(), pw)[0]
        Hc, Wc = ivc.canvas_of(v)
        want = np.zeros((n, Hc, Wc), dtype=np.uint8)
        want[:, :ph, :pw] = planes
        assert np.array_equal(t["masks"].cpu().numpy(), want)
        assert want[:2].any(axis=(1, 2)).all()                            # the corner triangle may leave the crop
        assert np.array_equal(t["boxes"].cpu().numpy(), ivc.bitmask_boxes(want)[0])
    # the vertex map itself, by hand: flip_in x -> 33 - x, resize x 25 / 33, y 30 / 40
    got = im.transform_polygons([[4.0, 3.0, 28.5, 6.0, 20.0, 31.0]], views[1], hw)[0]
    assert np.array_equal(got, np.array([(33 - 4.0) * (25 / 33), 3.0 * (30 / 40), (33 - 28.5) * (25 / 33),
                                         6.0 * (30 / 40), (33 - 20.0) * (25 / 33), 31.0 * (30 / 40)]))


def mixed_routes_keep_annotation_order(device):
    hw = (40, 33)
    m = ivc.case_masks(hw, ("blob", "noise"))
    anns = [{"segmentation": POLYS[0], "category_id": 1}, {"segmentation": to_rle(m[0]), "category_id": 2},
            {"segmentation": POLYS[1], "category_id": 3}, {"segmentation": m[1], "category_id": 4}]
    view = View(size=(60, 50), crop=(5, 8, 48, 40), canvas=(64, 64), fill=128)
    t = instance_mapper()([(image(hw, 0).to(device), anns)], views=[view])["instances"][0]
    only_poly = instance_mapper()([(image(hw, 0).to(device), [anns[0], anns[2]])], views=[view])["instances"][0]
    assert t["labels"].tolist() == [1, 2, 3, 4]
    assert torch.equal(t["masks"][[0, 2]], only_poly["masks"]) and torch.equal(t["boxes"][[0, 2]], only_poly["boxes"])
    want_m, want_b = dense_route([m[0], m[1]], view, device)
    assert torch.equal(t["masks"][[1, 3]], want_m) and torch.equal(t["boxes"][[1, 3]], want_b)


def lsj_filters_degenerate_rows(device):
    """A 48-pixel crop of a 2x up-scaled image from offset (32, 18): the masks left of or above it are dropped."""
    hw = (40, 33)
    mapper = im.COCOInstanceLSJMapper(image_size=48, min_scale=0.5, max_scale=2.0, pixel_mean=MEAN, pixel_std=STD)
    masks = np.zeros((5, 40, 33), dtype=np.uint8)
    masks[0, 2:6, 1:5] = 1                  # above and left of the window: empty
    masks[1, 20:30, 12:20] = 1              # inside
    masks[2, 0:40, 0:9] = 1                 # left of it (x < 18 after the 2x resize means source x < 9): empty
    masks[3, 16, 9] = 1                     # one source pixel at the window's corner: 2 x 2 pixels, kept
    masks[4, 39, 32] = 1                    # the last pixel: the window's last 2 x 2 pixels (rows 78, 79), kept
    anns = [{"segmentation": to_rle(m), "category_id": j} for j, m in enumerate(masks)]
    view = View(size=(80, 66), crop=(32, 18, 48, 48), canvas=(48, 48), flip_in=False, fill=128)
    smp = [(image(hw, 0).to(device), anns), (image((20, 24), 1).to(device), [])]
    views = [view, im.lsj_view(20, 24, 48, 1.0, 0.5, True, source=1)]
    res = mapper(smp, views=views)
    dm, db = dense_route(list(masks), view, device)
    keep = ((db[:, 2] - db[:, 0] > 1e-5) & (db[:, 3] - db[:, 1] > 1e-5)).cpu()
    assert keep.tolist() == [False, True, False, True, True]
    t = res["instances"][0]
    assert t["labels"].tolist() == [1, 3, 4] and torch.equal(t["masks"], dm[keep.to(device)])
    assert torch.equal(t["boxes"], db[keep.to(device)])
    assert res["instances"][1]["labels"].numel() == 0 and res["instances"][1]["masks"].shape == (0, 48, 48)
    # the padding mask against a resized plane of ones
    for i, (s, _) in enumerate(smp):
        import dataclasses
        ones = torch.ones((1,) + tuple(s.shape[:2]), dtype=torch.uint8, device=device)
        shown = label_views([ones], [dataclasses.replace(views[i], source=0)], seg_pad=0)[0][0, 0]
        assert torch.equal(res["padding_mask"][i], shown == 0)
    assert res["padding_mask"].dtype == torch.bool and not bool(res["padding_mask"][0].any())
    assert bool(res["padding_mask"][1].any())
    drawn = mapper(smp, np.random.default_rng(11))                        # and a drawn batch runs
    assert drawn["images"].shape == (2, 3, 48, 48) and all(v.canvas == (48, 48) for v in drawn["views"])


def sample_clip_frames_rule():
    rng = np.random.default_rng(0)
    for n, interval in ((5, 4), (10, 4), (11, 10), (20, 10), (21, 15), (30, 15), (31, 20), (40, 20), (41, 36),
                        (100, 36)):
        for _ in range(20):
            ref, tgt = im.sample_clip_frames(n, rng)
            assert tgt - ref == interval and 0 <= ref < n - interval
    for n in (1, 4):
        try:
            im.sample_clip_frames(n, rng)
        except ValueError:
            continue
        raise AssertionError(f"a video of {n} frames was accepted")


def video_mapper():
    return im.VideoInstanceTrainMapper(min_sizes=(40, 48), max_size=80, sample_style="choice_by_clip",
                                       random_flip="flip_by_clip", augmentations=(), num_frames=2,
                                       num_classes=NUM_CLASSES, pixel_mean=MEAN, pixel_std=STD)


def video_clips(device):
    hw = (40, 70)
    m = ivc.case_masks(hw, ("blob", "noise", "blob", "first"), seed=4)
    f0 = [{"id": 7, "category_id": 3, "segmentation": to_rle(m[0])},
          {"id": 2, "category_id": 5, "segmentation": to_rle(m[1])},
          {"id": 9, "category_id": 1, "segmentation": to_rle(np.zeros(hw, np.uint8))}]     # present, but empty
    f1 = [{"id": 7, "category_id": 3, "segmentation": to_rle(m[2])},
          {"id": 2, "category_id": 5, "segmentation": None},                                # absent
          {"id": 9, "category_id": 1, "segmentation": to_rle(m[3])},
          {"id": 4, "category_id": 8, "segmentation": to_rle(m[1]), "iscrowd": 1}]          # a crowd: dropped
    dense = [{7: m[0], 2: m[1], 9: np.zeros(hw, np.uint8)}, {7: m[2], 9: m[3]}]
    clip = ([image(hw, 0).to(device), image(hw, 1).to(device)], [f0, f1])
    other = ([image((30, 44), 2).to(device), image((30, 44), 3).to(device)], [[], []])      # a clip without instances
    return [clip, other], dense


def video_dummies_and_ids(device):
    clips, dense = video_clips(device)
    out = video_mapper()(clips, np.random.default_rng(5))
    assert len(out) == 2 and out[0]["images"].shape[:2] == (2, 3)
    frames = out[0]["instances"]
    cls = {7: 3, 2: 5, 9: 1}
    targets = []
    for t, f in enumerate(frames):
        ids = [2, 7, 9]                                                   # ascending
        masks = [dense[t].get(i, np.zeros((40, 70), np.uint8)) for i in ids]
        wm, wb = dense_route(masks, out[0]["views"][t], device)
        assert torch.equal(f["masks"], wm) and torch.equal(f["boxes"], wb)
        assert f["image_size"] == ivc.canvas_of(out[0]["views"][t]) == tuple(wm.shape[1:])
        empty = [not bool(x.any()) for x in wm]
        assert f["labels"].tolist() == [cls[i] if i in dense[t] else NUM_CLASSES for i in ids]
        assert f["ids"].tolist() == [-1 if (i not in dense[t] or e) else i for i, e in zip(ids, empty)]
        targets.append({"boxes": wb, "labels": f["labels"].clone(), "ids": f["ids"].clone(), "masks": wm,
                        "image_size": f["image_size"]})
    assert frames[0]["ids"].tolist()[2] == -1 and frames[0]["labels"].tolist()[2] == 1     # emptied, class kept
    assert frames[1]["ids"].tolist()[0] == -1 and frames[1]["labels"].tolist()[0] == NUM_CLASSES   # the dummy
    assert all(f["masks"].shape[0] == 0 and f["ids"].numel() == 0 for f in out[1]["instances"])
    # the targets run through the two preparations as they are and give what the dense-route targets give
    Hp, Wp = out[0]["images"].shape[-2:]
    got = prepare_video_targets([out[0]], (Hp, Wp), 2)
    want = prepare_video_targets([targets], (Hp, Wp), 2)
    for a, b in zip(got, want):
        assert all(torch.equal(a[k], b[k]) for k in ("labels", "ids", "masks"))
    return out, targets


def video_weaksup_targets(device):
    out, targets = video_dummies_and_ids(device)
    org = [f.permute(2, 0, 1) for f in video_clips(device)[0][0][0]]
    # frames of one size whose padded size is a multiple of the stride
    got = prepare_video_weaksup_targets([out[0]], org, num_frames=2, size_divisibility=32)
    want = prepare_video_weaksup_targets([targets], org, num_frames=2, size_divisibility=32)
    for a, b in zip(got, want):
        for k in ("labels", "ids", "box_masks", "masks", "left_bounds", "right_bounds", "top_bounds", "bottom_bounds"):
            assert torch.equal(a[k], b[k]), k
