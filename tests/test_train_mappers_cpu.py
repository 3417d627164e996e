"""bm2f_amd.train_mappers on CPU tensors: the drawn geometry, the label batch against Pillow's NEAREST under the same
geometry, the targets, and the by-clip counters of video_clip_views."""
import numpy as np
import pytest
import torch

import color_aug_cases as cc
from bm2f_amd import (ColorAug, PanopticTrainMapper, SemanticTrainMapper, View, image_views, panoptic_targets,
                      resize_shortest_edge_size, semantic_targets, semantic_train_view, video_clip_views)

MIN_SIZES = (32, 40, 48, 77)


def samples(n=3, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = (40, 56) if i % 2 == 0 else (61, 45)
        lab = rng.integers(0, 7, (h, w)).astype(np.uint8)
        lab[: h // 4, : w // 3] = 255
        out.append((torch.from_numpy(cc.random_image(h, w, 40 + i)), torch.from_numpy(lab)))
    return out


def mapper(cls=SemanticTrainMapper, **kw):
    args = dict(min_sizes=MIN_SIZES, max_size=96, crop_size=(32, 32), ignore_label=255, num_classes=7,
                pixel_mean=cc.MEAN, pixel_std=cc.STD, img_format="RGB", size_divisibility=32)
    args.update(kw)
    return cls(**args)


def test_view_sizes_and_crop_windows():
    rng = np.random.default_rng(0)
    seen_sizes, seen_flip = set(), set()
    for _ in range(200):
        h, w = int(rng.integers(20, 90)), int(rng.integers(20, 90))
        v = semantic_train_view(h, w, min_sizes=MIN_SIZES, max_size=96, crop_size=(32, 40), flip=True, color=True,
                                rng=rng, size_divisibility=48, img_format="RGB")
        assert v.size in {resize_shortest_edge_size(h, w, s, 96) for s in MIN_SIZES}
        y0, x0, ch, cw = v.crop
        assert (ch, cw) == (min(32, v.size[0]), min(40, v.size[1]))
        assert 0 <= y0 and y0 + ch <= v.size[0] and 0 <= x0 and x0 + cw <= v.size[1]
        assert v.canvas == (48, 48) and v.fill == 128 and not v.flip_in
        assert isinstance(v.color, ColorAug) and v.color.swap_rb
        seen_sizes.add(min(v.size))
        seen_flip.add(v.flip_out)
    assert seen_flip == {False, True} and len(seen_sizes) >= 3
    fixed = ColorAug((("ssd_hue", 3),))
    v = semantic_train_view(40, 56, min_sizes=(32,), max_size=96, crop_size=None, flip=False, color=fixed,
                            rng=np.random.default_rng(0))
    assert v == View(size=(32, 45), crop=(0, 0, 32, 45), canvas=(32, 45), fill=128, color=fixed)
    with pytest.raises(ValueError, match="SINGLE_CATEGORY_MAX_AREA"):
        mapper(single_category_max_area=0.75)


def test_label_batch_is_pillow_nearest_under_the_same_geometry():
    Image = pytest.importorskip("PIL.Image")
    s = samples()
    out = mapper()(s, np.random.default_rng(3))
    assert tuple(out["images"].shape) == (3, 3, 32, 32) and tuple(out["labels"].shape) == (3, 1, 32, 32)
    assert out["labels"].dtype == torch.uint8 and out["image_sizes"] == [(32, 32)] * 3
    for i, ((img, lab), v) in enumerate(zip(s, out["views"])):
        r = np.asarray(Image.fromarray(lab.numpy()).resize((v.size[1], v.size[0]), Image.NEAREST))
        y0, x0, ch, cw = v.crop
        win = r[y0:y0 + ch, x0:x0 + cw]
        win = win[:, ::-1] if v.flip_out else win
        want = np.full((32, 32), 255, np.uint8)
        want[:ch, :cw] = win
        assert np.array_equal(out["labels"][i, 0].numpy(), want), i
        # the image under the same geometry: Pillow's BILINEAR, then the view's colour, fill 128, normalised
        pim = np.asarray(Image.fromarray(img.numpy()).resize((v.size[1], v.size[0]), Image.BILINEAR))
        pim = pim[y0:y0 + ch, x0:x0 + cw]
        pim = np.ascontiguousarray(pim[:, ::-1] if v.flip_out else pim)
        from bm2f_amd.color_aug import apply_color
        canvas = np.full((32, 32, 3), 128, np.uint8)
        canvas[:ch, :cw] = apply_color(pim, v.color)
        x = torch.from_numpy(canvas).permute(2, 0, 1).float()
        x = (x - torch.tensor(cc.MEAN).view(3, 1, 1)) / torch.tensor(cc.STD).view(3, 1, 1)
        assert torch.equal(out["images"][i], x), i


def test_targets_are_semantic_targets_of_the_label_batch():
    s = samples()
    out = mapper()(s, np.random.default_rng(4))
    want = semantic_targets([out["labels"][i, 0] for i in range(3)], 255, 7)
    assert len(out["targets"]) == 3
    for g, w in zip(out["targets"], want):
        assert sorted(g) == sorted(w) == ["areas", "ids", "label_map", "labels"]
        for k in w:
            assert torch.equal(g[k], w[k]), k
        assert 255 not in g["ids"].tolist() and int(g["areas"].sum()) == int((g["label_map"] != 255).sum())
    # the same generator state gives the same views; given views are used as they are
    again = mapper()(s, np.random.default_rng(4))
    assert again["views"] == out["views"] and torch.equal(again["images"], out["images"])
    given = mapper()(s, views=out["views"])
    assert torch.equal(given["images"], out["images"]) and torch.equal(given["labels"], out["labels"])
    off = mapper(color_aug_ssd=False)(s, np.random.default_rng(4))
    assert all(v.color is None for v in off["views"])


def test_panoptic_mapper():
    rng = np.random.default_rng(6)
    s = []
    for img, _ in samples(2):
        h, w = img.shape[:2]
        pan = torch.from_numpy((rng.integers(1, 4, (h, w)) * 1000 + 7).astype(np.int32))
        infos = [{"id": k * 1000 + 7, "category_id": k + 10, "iscrowd": int(k == 3)} for k in (1, 2, 3)]
        s.append((img, pan, infos))
    m = mapper(PanopticTrainMapper)
    out = m(s, np.random.default_rng(8))
    images, _ = image_views([x[0] for x in s], out["views"], pixel_mean=cc.MEAN, pixel_std=cc.STD,
                            out_dtype=torch.float32)
    assert torch.equal(out["images"], images)
    assert out["labels"].dtype == torch.int32 and set(out["labels"].unique().tolist()) <= {0, 1007, 2007, 3007}
    want = panoptic_targets([out["labels"][i, 0] for i in range(2)], [x[2] for x in s])
    for g, w in zip(out["targets"], want):
        assert g["labels"].tolist() == [11, 12] and g["ids"].tolist() == [1007, 2007]
        for k in w:
            assert torch.equal(g[k], w[k]), k


def test_video_clip_views_counters():
    shapes = [(40, 56)] * 12
    for style, flip in (("range_by_clip", "flip_by_clip"), ("choice_by_clip", "flip_by_clip")):
        sizes_differ = flips_differ = False
        for seed in range(8):
            views = video_clip_views(shapes, min_sizes=(24, 48) if "range" in style else (24, 32, 40, 48),
                                     max_size=96, sample_style=style, random_flip=flip,
                                     augmentations=["brightness", "contrast", "saturation"], clip_frame_cnt=4,
                                     rng=np.random.default_rng(seed))
            assert [v.source for v in views] == list(range(12))
            for c in range(3):
                clip = views[4 * c:4 * c + 4]
                assert len({v.size for v in clip}) == 1 and len({v.flip_out for v in clip}) == 1
                assert len({v.color for v in clip}) == 4              # the blends are redrawn per frame
                assert [n for n, _ in clip[0].color.ops] == ["brightness", "contrast", "saturation"]
            sizes_differ |= len({v.size for v in views}) > 1
            flips_differ |= len({v.flip_out for v in views}) > 1
            for v in views:
                assert v.size in {resize_shortest_edge_size(40, 56, s, 96) for s in range(24, 49)}
        assert sizes_differ and flips_differ
    per_frame = video_clip_views(shapes, min_sizes=(24, 48), max_size=96, sample_style="range",
                                 random_flip="horizontal", augmentations=[], clip_frame_cnt=4,
                                 rng=np.random.default_rng(1))
    assert any(len({v.size for v in per_frame[4 * c:4 * c + 4]}) > 1 for c in range(3))
    assert any(len({v.flip_out for v in per_frame[4 * c:4 * c + 4]}) > 1 for c in range(3))
    assert all(v.color is None for v in per_frame)
    none = video_clip_views(shapes[:3], min_sizes=(32,), max_size=96, sample_style="choice", random_flip="none",
                            augmentations=["contrast"], clip_frame_cnt=3, rng=np.random.default_rng(1))
    assert not any(v.flip_out for v in none) and all(v.size == (32, 45) for v in none)
    for bad in (dict(random_flip="vertical"), dict(augmentations=["rotation"]), dict(sample_style="fixed")):
        kw = dict(min_sizes=(32,), max_size=96, sample_style="choice", random_flip="none", augmentations=[],
                  clip_frame_cnt=2, rng=np.random.default_rng(0))
        kw.update(bad)
        with pytest.raises(ValueError):
            video_clip_views(shapes[:2], **kw)
    # the views run: one image_views call for the clip, contrast means per frame
    srcs = [torch.from_numpy(cc.random_image(40, 56, 60 + i)) for i in range(3)]
    batch, sizes = image_views(srcs, none, out_dtype=torch.uint8)
    assert tuple(batch.shape) == (3, 3, 32, 45) and sizes == [(32, 45)] * 3
