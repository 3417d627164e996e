"""bm2f_amd.color_aug (the numpy definition of the colour augmentations) against the literal numpy expressions of
detectron2's ``convert`` / ``BlendTransform``, OpenCV's HSV anchors and invariants, and tests/golden/color_aug.npz; and
image_views on CPU tensors with ``View.color``.  Every comparison is exact equality.  cv2 and detectron2 are not used:
the HSV restatement is held to its anchors and invariants only."""
import dataclasses
import functools
import itertools

import numpy as np
import pytest
import torch
from conftest import golden

import color_aug_cases as cc
import image_view_cases as ivc
import image_view_checks as checks
from bm2f_amd import ColorAug, View, color_aug as ca, draw_color_aug_ssd, draw_video_photometric, image_views


@functools.lru_cache(maxsize=None)
def fixture():
    z = golden("color_aug.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def sweep():
    return cc.sweep_image()


def images():
    small = fixture()["small"]
    return [small, cc.random_image(61, 47, 2), np.zeros((3, 4, 3), np.uint8), np.full((2, 5, 3), 255, np.uint8)]


def test_convert_equals_the_literal_expression():
    for img in images():
        for a, b in ((0.5, 0), (1.5, 0), (1, 32), (1, -32), (1, 31.999), (0.731, 0), (1.4999, -12.3)):
            assert np.array_equal(ca.convert(img, a, b), cc.literal_convert(img, a, b)), (a, b)
        assert np.array_equal(ca.ssd_brightness(img, -32), cc.literal_convert(img, beta=-32))
        assert np.array_equal(ca.ssd_contrast(img, 1.5), cc.literal_convert(img, alpha=1.5))
    fx = fixture()
    for a, b in ((0.5, 0), (1.5, 0), (1, 32), (1, -32)):
        assert np.array_equal(ca.convert(fx["small"], a, b), fx[f"literal_convert_{a}_{b}"])


def test_blends_equal_the_literal_expressions():
    """Under the installed numpy: fp32 for brightness, fp64 for contrast and saturation (tests pin the dtypes too)."""
    for img in images():
        for w in (0.9, 1.1, 1.0, 0.9731, 1.0517):
            lit = cc.literal_blends(img, w)
            assert np.array_equal(ca.blend_brightness(img, w), lit["brightness"]), w
            assert np.array_equal(ca.blend_contrast(img, w), lit["contrast"]), w
            assert np.array_equal(ca.blend_saturation(img, w), lit["saturation"]), w
    fx = fixture()
    for w in (0.9, 1.1):
        for n, f in (("brightness", ca.blend_brightness), ("contrast", ca.blend_contrast),
                     ("saturation", ca.blend_saturation)):
            assert np.array_equal(f(fx["small"], w), fx[f"literal_{n}_{w}"]), (n, w)
    img = images()[1]
    f32 = img.astype(np.float32)
    assert ((1 - 0.9) * 0 + 0.9 * f32).dtype == np.float32
    assert ((1 - 0.9) * img.mean() + 0.9 * f32).dtype == np.float64
    assert ((1 - 0.9) * img.dot([0.299, 0.587, 0.114])[:, :, None] + 0.9 * f32).dtype == np.float64


def test_grayscale_is_the_fma_chain_of_dot():
    """``grayscale`` equals ``img.dot`` under the installed numpy / BLAS, and the exactly rounded fma chain always."""
    from fractions import Fraction as Fr
    img = images()[1]
    g = ca.grayscale(img)
    assert g.dtype == np.float64 and np.array_equal(g, img.dot([0.299, 0.587, 0.114]))
    for (c0, c1, c2), got in list(zip(img.reshape(-1, 3).tolist(), g.reshape(-1).tolist()))[:500]:
        inner = float(Fr(c1) * Fr(0.587) + Fr(c0 * 0.299))
        assert got == float(Fr(c2) * Fr(0.114) + Fr(inner))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(ca.grayscale(grey), grey.dot([0.299, 0.587, 0.114]))


def test_exact_mean_is_numpy_mean():
    for img in images():
        assert ca.exact_mean(img.sum(dtype=np.int64), img.size) == img.mean()


def test_hsv_anchors():
    px = np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0]]], dtype=np.uint8)
    assert ca.bgr2hsv(px).tolist() == [[[0, 255, 255], [60, 255, 255], [120, 255, 255]]]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    hsv = ca.bgr2hsv(grey)
    assert (hsv[..., :2] == 0).all() and np.array_equal(hsv[..., 2], grey[..., 0])
    assert np.array_equal(ca.hsv2bgr(np.array([[[0, 255, 255], [60, 255, 255], [120, 255, 255]]], np.uint8)), px)
    sdiv, hdiv = ca.hsv_tables()
    assert sdiv[0] == 0 and hdiv[0] == 0 and sdiv[255] == 4096 and sdiv[1] == 255 << 12 and hdiv[1] == 30 << 12
    assert hdiv[255] == 482 and sdiv.dtype == np.int32 and sdiv.shape == hdiv.shape == (256,)
    assert np.array_equal(ca.bgr2hsv(fixture()["small"]), fixture()["small_hsv"])


def test_hsv_round_trip_keeps_grey_and_black_and_h_stays_below_180():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)          # all 256 greys beside the sweep
    s = np.concatenate([sweep(), grey], axis=1)
    hsv = ca.bgr2hsv(s)
    assert int(hsv[..., 0].max()) < 180
    keep = (hsv[..., 1] == 0) | (hsv[..., 2] == 0)
    assert keep.sum() >= 256 and np.array_equal(ca.hsv2bgr(hsv)[keep], s[keep])
    # v is the maximum and survives every round trip; a zero hue shift is the plain round trip
    assert np.array_equal(ca.hsv2bgr(hsv).max(-1), s.max(-1))
    assert np.array_equal(ca.ssd_hue(s, 0), ca.hsv2bgr(hsv))


def test_hue_shift_and_back_is_the_identity_in_h():
    hsv = ca.bgr2hsv(sweep())
    h = hsv[..., 0].astype(np.int64)
    assert {0, 179} <= set(np.unique(h).tolist())
    for d in (1, 18, -18, 179, 180, -200):
        there = (h + d) % 180
        assert there.min() >= 0 and there.max() < 180
        assert np.array_equal((there - d) % 180, h), d
    # through the operation itself: H of the shifted image's HSV input is (H + d) mod 180, read back from a grid of
    # fully saturated colours, where the conversion back and forth is exact
    pure = np.zeros((1, 180, 3), np.uint8)
    pure[..., 0], pure[..., 1], pure[..., 2] = np.arange(180), 255, 255
    bgr = ca.hsv2bgr(pure)
    assert np.array_equal(ca.bgr2hsv(bgr), pure)
    for d in (18, -18, 1, -1):
        shifted = ca.bgr2hsv(ca.ssd_hue(bgr, d))
        assert np.array_equal(shifted[0, :, 0], (np.arange(180) + d) % 180), d
        assert np.array_equal(ca.bgr2hsv(ca.ssd_hue(ca.ssd_hue(bgr, d), -d)), pure), d


STEPS = {"ssd_brightness": 20.5, "ssd_contrast": 0.83, "ssd_saturation": 1.3, "ssd_hue": -7}


def test_both_orders_and_every_subset_compose_the_single_steps():
    img = fixture()["small"]
    single = {"ssd_brightness": ca.ssd_brightness, "ssd_contrast": ca.ssd_contrast,
              "ssd_saturation": ca.ssd_saturation, "ssd_hue": ca.ssd_hue}
    orders = (("ssd_brightness", "ssd_contrast", "ssd_saturation", "ssd_hue"),
              ("ssd_brightness", "ssd_saturation", "ssd_hue", "ssd_contrast"))
    seen = set()
    for order in orders:
        for r in range(5):
            for subset in itertools.combinations(order, r):
                want = img
                for n in subset:
                    want = single[n](want, STEPS[n])
                got = ca.apply_color(img, ColorAug(tuple((n, STEPS[n]) for n in subset)))
                assert np.array_equal(got, want), subset
                seen.add(subset)
    assert len(seen) == 22      # 16 subsets, 6 of them in two orders (contrast before or after saturation / hue)


def test_rgb_format_swaps_the_channels_around_the_bgr_result():
    img = fixture()["small"]
    for name in ("ssd_order_a", "ssd_order_b_rgb", "ssd_saturation_137", "ssd_hue_m18"):
        ops = cc.COLOR_CASES[name].ops
        bgr = ca.apply_color(np.ascontiguousarray(img[..., ::-1]), ColorAug(ops, swap_rb=False))
        assert np.array_equal(ca.apply_color(img, ColorAug(ops, swap_rb=True)), bgr[..., ::-1]), name
    assert not np.array_equal(ca.apply_color(img, ColorAug(cc.COLOR_CASES["ssd_hue_m18"].ops, swap_rb=True)),
                              ca.apply_color(img, cc.COLOR_CASES["ssd_hue_m18"]))


def test_definition_equals_the_fixture():
    fx = fixture()
    assert str(fx["numpy"]).split(".")[0] == np.__version__.split(".")[0], "the fixture was recorded under another major"
    for name, aug in cc.COLOR_CASES.items():
        assert np.array_equal(ca.apply_color(fx["small"], aug), fx[f"small_{name}"]), name
    for name in ("ssd_order_a", "video_all", "ssd_saturation_05"):
        got = ca.apply_color(sweep(), cc.COLOR_CASES[name])[::cc.SWEEP_STRIDE, ::cc.SWEEP_STRIDE]
        assert np.array_equal(got, fx[f"sweep_{name}"]), name


def test_color_aug_record_and_table_row():
    with pytest.raises(ValueError, match="unknown"):
        ColorAug((("gamma", 1.0),))
    with pytest.raises(ValueError, match="at most 4"):
        ColorAug((("brightness", 1.0),) * 5)
    with pytest.raises(ValueError, match="one \"contrast\""):
        ColorAug((("contrast", 1.0), ("contrast", 0.9)))
    aug = cc.MEAN_AUGS["contrast_after"]
    assert aug.contrast_index == 1 and not aug.needs_hsv and cc.COLOR_CASES["ssd_hue_p18"].needs_hsv
    row = ca.encode(aug)
    assert row.shape == (ca.FIELDS,) and row.dtype == np.float64 and row[:3].tolist() == [3, 0, 1]
    assert row[4:13].tolist() == [1, 1.1, -0.0, 4, 1 - 1.1, 1.1, 5, 1 - 0.9, 0.9]
    assert ca.encode(None)[2] == -1 and ca.encode(None)[0] == 0
    assert hash(aug) == hash(dataclasses.replace(aug)) and View(size=(1, 1)).color is None


def test_draws_follow_the_distributions():
    rng = np.random.default_rng(0)
    draws = [draw_color_aug_ssd(rng) for _ in range(400)]
    orders = set()
    for d in draws:
        names = [n for n, _ in d.ops]
        assert len(names) == len(set(names)) and not d.swap_rb
        if "ssd_brightness" in names:
            assert names[0] == "ssd_brightness"
        rest = [n for n in names if n != "ssd_brightness"]
        assert rest in ([x for x in o if x in rest] for o in (("ssd_contrast", "ssd_saturation", "ssd_hue"),
                                                              ("ssd_saturation", "ssd_hue", "ssd_contrast")))
        if "ssd_contrast" in rest and len(rest) > 1:
            orders.add(rest.index("ssd_contrast") == 0)
        for n, v in d.ops:
            lo, hi = {"ssd_brightness": (-32, 32), "ssd_contrast": (0.5, 1.5), "ssd_saturation": (0.5, 1.5),
                      "ssd_hue": (-18, 18)}[n]
            assert lo <= v <= hi and (n != "ssd_hue" or isinstance(v, int))
    assert orders == {True, False}
    assert {len(d.ops) for d in draws} == {0, 1, 2, 3, 4}
    assert {v for d in draws for n, v in d.ops if n == "ssd_hue"} >= {-18, 18}
    assert draw_color_aug_ssd(rng, img_format="RGB").swap_rb
    v = draw_video_photometric(rng, ["saturation", "brightness"])
    assert [n for n, _ in v.ops] == ["brightness", "saturation"] and all(0.9 <= w <= 1.1 for _, w in v.ops)
    assert draw_video_photometric(rng, []).ops == ()
    with pytest.raises(ValueError, match="rotation"):
        draw_video_photometric(rng, ["rotation"])


# ------------------------------------------------------------------------------------------------ image_views
@pytest.mark.parametrize("case", ivc.IMAGE_CASES, ids=lambda c: c["name"])
def test_color_none_is_the_output_before_the_change(case):
    """The cases of the existing image-view tests with ``color=None`` spelled out, and with an empty operation list:
    still Pillow's recorded output."""
    src = torch.from_numpy(ivc.image_source(case))
    for color in (None, ColorAug()):
        got, _ = image_views([src], [dataclasses.replace(checks.view_of(case), color=color)], out_dtype=torch.uint8)
        assert ivc.matches(checks.fixture(), case["name"], got[0].numpy()), case["name"]


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_fill_and_pad_stay_uncoloured(fam):
    aug = cc.COLOR_CASES[fam]
    src = cc.random_image(*cc.GEO_SOURCE, 3)
    t = torch.from_numpy(src)
    for vname in cc.GEO_VIEWS:
        view = cc.geo_view(vname, aug)
        got, sizes = image_views([t], [view], out_dtype=torch.uint8, size_divisibility=cc.GEO_PAD, pad_value=7)
        assert np.array_equal(got[0].numpy(), fixture()[f"geo_{vname}_{fam}"]), vname
        plain, _ = image_views([t], [dataclasses.replace(view, color=None)], out_dtype=torch.uint8,
                               size_divisibility=cc.GEO_PAD, pad_value=7)
        shown, _ = image_views([torch.full_like(t, 255)], [dataclasses.replace(view, color=None, fill=0)],
                               out_dtype=torch.uint8, size_divisibility=cc.GEO_PAD, pad_value=0)
        inside = (shown == 255).all(1)[0]
        Hc, Wc = sizes[0]
        assert (got[0, :, Hc:] == 7).all() and (got[0, :, :, Wc:] == 7).all()
        canvas_fill = ~inside[:Hc, :Wc]
        assert (got[0, :, :Hc, :Wc][:, canvas_fill] == 128).all() and torch.equal(got[0][:, ~inside], plain[0][:, ~inside])
        # the shown pixels are the operations on the plain view's shown pixels, mean over exactly them
        px = plain[0][:, inside].T.numpy()
        assert np.array_equal(got[0][:, inside].T.numpy(), ca.apply_color(np.ascontiguousarray(px)[None], aug)[0]), vname
        norm, _ = image_views([t], [view], out_dtype=torch.float32, pixel_mean=cc.MEAN, pixel_std=cc.STD,
                              size_divisibility=cc.GEO_PAD, pad_value=-3.5)
        want = (got[0].float() - torch.tensor(cc.MEAN).view(3, 1, 1)) / torch.tensor(cc.STD).view(3, 1, 1)
        assert torch.equal(norm[0, :, :Hc, :Wc], want[:, :Hc, :Wc]) and (norm[0, :, Hc:] == -3.5).all()


def test_contrast_mean_cases_equal_the_fixture():
    for mname, (shape, view) in cc.MEAN_CASES.items():
        src = torch.from_numpy(cc.random_image(*shape, 17))
        for aname, aug in cc.MEAN_AUGS.items():
            got, _ = image_views([src], [dataclasses.replace(view, color=aug)], out_dtype=torch.uint8)
            assert np.array_equal(got[0].numpy(), fixture()[f"mean_{mname}_{aname}"]), (mname, aname)
