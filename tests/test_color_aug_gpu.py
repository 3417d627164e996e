"""``m2f_image_views_color`` and ``m2f_image_views_sum`` (csrc/image_views.hip) on the device against the numpy
definition of bm2f_amd/color_aug.py, computed live through image_views on CPU tensors, and against its recorded outputs
(tests/golden/color_aug.npz).  Every comparison is exact equality."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
from conftest import golden

import color_aug_cases as cc
from bm2f_amd import SemanticTrainMapper, View, _native, color_aug as ca, image_views

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    z = golden("color_aug.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def sweep():
    return cc.sweep_image()


@functools.lru_cache(maxsize=None)
def geo_source():
    return cc.random_image(*cc.GEO_SOURCE, 3)


def bits(t):
    return t.cpu().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def both(srcs, views, device, **kw):
    """(device output, CPU-definition output) of one image_views call, sizes compared."""
    srcs = [torch.from_numpy(np.ascontiguousarray(s)) for s in srcs]
    want, wsizes = image_views(srcs, views, **kw)
    got, gsizes = image_views([s.to(device) for s in srcs], views, **kw)
    assert gsizes == wsizes and got.shape == want.shape and got.dtype == want.dtype
    return got, want


@pytest.mark.parametrize("name", list(cc.COLOR_CASES))
def test_colour_sweep(name, device):
    """All (r, g) pairs at six b values, at the source's own size (no resize): uint8 and fp32 normalised."""
    aug = cc.COLOR_CASES[name]
    view = [View(size=(256, 1536), color=aug)]
    got, want = both([sweep()], view, device, out_dtype=torch.uint8)
    assert torch.equal(got.cpu(), want), name
    hwc = got[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(hwc, ca.apply_color(sweep(), aug))
    assert np.array_equal(hwc[::cc.SWEEP_STRIDE, ::cc.SWEEP_STRIDE], fixture()[f"sweep_{name}"]), name
    got, want = both([sweep()], view, device, out_dtype=torch.float32, pixel_mean=cc.MEAN, pixel_std=cc.STD)
    assert torch.equal(bits(got), bits(want)), name


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_geometry_with_colour_leaves_fill_and_pad(fam, device):
    aug = cc.COLOR_CASES[fam]
    for vname in cc.GEO_VIEWS:
        view = cc.geo_view(vname, aug)
        got, want = both([geo_source()], [view], device, out_dtype=torch.uint8, size_divisibility=cc.GEO_PAD,
                         pad_value=7)
        assert torch.equal(got.cpu(), want), vname
        assert np.array_equal(got[0].cpu().numpy(), fixture()[f"geo_{vname}_{fam}"]), vname
        # fill and pad are where the uncoloured call has them, and hold the same bytes
        plain, _ = image_views([torch.from_numpy(geo_source()).to(device)], [dataclasses.replace(view, color=None)],
                               out_dtype=torch.uint8, size_divisibility=cc.GEO_PAD, pad_value=7)
        shown, _ = image_views([torch.full(cc.GEO_SOURCE + (3,), 255, dtype=torch.uint8, device=device)],
                               [dataclasses.replace(view, color=None, fill=0)], out_dtype=torch.uint8,
                               size_divisibility=cc.GEO_PAD, pad_value=0)
        outside = shown != 255
        assert bool(outside.any()) and torch.equal(got[outside], plain[outside]), vname
        got, want = both([geo_source()], [view], device, out_dtype=torch.float32, pixel_mean=cc.MEAN,
                         pixel_std=cc.STD, size_divisibility=cc.GEO_PAD, pad_value=-3.5)
        assert torch.equal(bits(got), bits(want)), vname


def test_five_views_two_sources_one_call(device, monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: calls.append(name) or real(name, *a))
    srcs = [geo_source(), cc.random_image(20, 30, 4)]
    views = [cc.geo_view("down_crop_past_flip_out", cc.COLOR_CASES["ssd_order_a"]),
             cc.geo_view("up_wide_canvas", None),
             View(size=(20, 30), source=1, color=cc.COLOR_CASES["video_all"]),
             View(size=(33, 47), source=1, flip_out=True, color=cc.COLOR_CASES["ssd_order_b_rgb"]),
             cc.geo_view("up_whole", cc.COLOR_CASES["video_saturation_09"])]
    dev_srcs = [torch.from_numpy(s).to(device) for s in srcs]
    got, sizes = image_views(dev_srcs, views, out_dtype=torch.uint8, size_divisibility=32, pad_value=9)
    assert calls == ["m2f_image_views_sum_workspace", "m2f_image_views_sum", "m2f_image_views_color"]
    want, wsizes = image_views([torch.from_numpy(s) for s in srcs], views, out_dtype=torch.uint8,
                               size_divisibility=32, pad_value=9)
    assert sizes == wsizes and torch.equal(got.cpu(), want)
    # the view without colour equals the plain entry point's output, and a call without a contrast blend is one launch
    plain, _ = image_views(dev_srcs, [views[1]], out_dtype=torch.uint8, size_divisibility=32, pad_value=9)
    assert torch.equal(got[1, :, :plain.shape[2], :plain.shape[3]], plain[0])
    del calls[:]
    image_views(dev_srcs, [views[0], views[1]], out_dtype=torch.uint8)
    image_views(dev_srcs, [views[1]], out_dtype=torch.uint8)
    assert calls == ["m2f_image_views_color", "m2f_image_views"]


@pytest.mark.parametrize("mname", list(cc.MEAN_CASES))
def test_contrast_mean_is_exact_and_repeatable(mname, device):
    shape, view = cc.MEAN_CASES[mname]
    src = cc.random_image(*shape, 17)
    for aname, aug in cc.MEAN_AUGS.items():
        v = [dataclasses.replace(view, color=aug)]
        got, want = both([src], v, device, out_dtype=torch.uint8)
        assert torch.equal(got.cpu(), want), (mname, aname)
        assert np.array_equal(got[0].cpu().numpy(), fixture()[f"mean_{mname}_{aname}"]), (mname, aname)
        again, _ = image_views([torch.from_numpy(src).to(device)], v, out_dtype=torch.uint8)
        assert torch.equal(again, got), (mname, aname)
        got, want = both([src], v, device, out_dtype=torch.float32, pixel_mean=cc.MEAN, pixel_std=cc.STD)
        assert torch.equal(bits(got), bits(want)), (mname, aname)


def test_view_sums_equal_the_integer_sum(device):
    """What m2f_image_views_sum leaves in its workspace: per view the exact integer sum of the shown pixels after the
    operations before the contrast blend, 0 for a view without one."""
    mod = __import__("bm2f_amd.image_views", fromlist=["_Plan"])
    src = geo_source()
    views = [View(size=(61, 89), color=cc.MEAN_AUGS["contrast_after"]), View(size=(23, 31)),
             View(size=(37, 53), color=cc.MEAN_AUGS["contrast_after_hue"])]
    plan = mod._Plan(views, [cc.GEO_SOURCE], image=True)
    rows = plan.rows.copy()
    rows[:, 3] = 3 * cc.GEO_SOURCE[1]
    t = torch.from_numpy(src).to(device)
    keep, rows_dev, tables_dev, colors_dev = mod._upload_plan(mod._with_rows(plan, rows), device)
    colors = np.ascontiguousarray(plan.colors)
    Hp, Wp = plan.padded(0)
    ws = _native.workspace("m2f_image_views_sum_workspace", mod._host_ptr(rows), 3, Hp, Wp, device=device,
                           dtype=torch.int64)
    _native.call("m2f_image_views_sum", t.data_ptr(), t.numel(), mod._host_ptr(rows), rows_dev, 3, tables_dev,
                 plan.tables.size, mod._host_ptr(colors), colors_dev, int(plan.hsv_off), Hp, Wp, ws.data_ptr(),
                 ws.numel(), _native.stream(device))
    want = []
    for v in views:
        r = mod._resize_bilinear_np(src, v.size)
        want.append(ca.color_sum(r, v.color) if v.color is not None else 0)
    assert ws[:3].cpu().tolist() == want


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_outputs(dtype, device):
    src = cc.random_image(3, 5, 17)
    for aug in (cc.COLOR_CASES["ssd_order_a"], cc.COLOR_CASES["video_all"]):
        got, want = both([src], [View(size=(3, 5), canvas=(4, 6), fill=128, color=aug)], device, out_dtype=dtype,
                         pixel_mean=cc.MEAN, pixel_std=cc.STD, size_divisibility=8, pad_value=-1.25)
        assert torch.equal(bits(got), bits(want))


def test_bad_colour_row_is_refused_before_any_launch(device):
    mod = __import__("bm2f_amd.image_views", fromlist=["_Plan"])
    img = torch.from_numpy(geo_source()).to(device)
    plan = mod._Plan([View(size=(19, 23), color=cc.COLOR_CASES["ssd_order_a"])], [cc.GEO_SOURCE], image=True)
    rows = plan.rows.copy()
    rows[0, 3] = 3 * cc.GEO_SOURCE[1]
    for column, value in ((0, 5.0), (4, 9.0), (5, float("nan")), (2, 1.0)):
        bad = mod._with_rows(plan, rows)
        bad.colors = plan.colors.copy()
        bad.colors[0, column] = value
        out = torch.full((1, 3, 19, 23), 0xA5, dtype=torch.uint8, device=device)
        with pytest.raises(_native.NativeError, match=r"code 3\).*view 0"):
            mod._launch_image(img.data_ptr(), img.numel(), bad, rows, out, None, None, 0.0)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()), column


def test_semantic_train_mapper_equals_the_cpu_path(device):
    rng = np.random.default_rng(23)
    samples = [(torch.from_numpy(cc.random_image(40, 56, 30 + i)),
                torch.from_numpy(rng.integers(0, 7, (40, 56)).astype(np.uint8))) for i in range(2)]
    samples[1][1][:9, :11] = 255
    mapper = SemanticTrainMapper(min_sizes=(32, 40, 48), max_size=96, crop_size=(32, 32), ignore_label=255,
                                 num_classes=7, pixel_mean=cc.MEAN, pixel_std=cc.STD, img_format="RGB",
                                 size_divisibility=32)
    want = mapper(samples, np.random.default_rng(5))
    got = mapper([(im.to(device), lab.to(device)) for im, lab in samples], np.random.default_rng(5))
    assert got["views"] == want["views"] and got["image_sizes"] == want["image_sizes"]
    assert any(v.color is not None and v.color.ops for v in got["views"])
    assert got["images"].device.type == "cuda" and torch.equal(bits(got["images"]), bits(want["images"]))
    assert torch.equal(got["labels"].cpu(), want["labels"])
    for g, w in zip(got["targets"], want["targets"]):
        assert sorted(g) == sorted(w)
        for k in w:
            assert torch.equal(g[k].cpu(), w[k]), k
