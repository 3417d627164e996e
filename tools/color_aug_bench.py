"""Wall time of the fused colour stage of the device input pipeline (m2f_image_views_color, bm2f_amd/image_views.py)
against the same call without colour and against two ways of doing the colour elsewhere, written to
profiles/color_aug.json.

    python tools/color_aug_bench.py [--reps N] [--out profiles/color_aug.json]

Routes, all ending with the fp32 normalised batch on the device after a synchronise:
  fused   one upload of the uint8 sources, one image_views call with View.color (for the video blends one
          m2f_image_views_sum launch more);
  plain   the same call with every View.color None: the cost of the colour stage is fused - plain;
  host    (a) the views as uint8 from the numpy definition on the host (image_views on CPU tensors, colour included),
          one upload of the finished batch, normalisation on the device;
  torch   (b) image_views to uint8 on the device, then the colour operations as torch tensor operations on the device
          (integer HSV with gathers from the two tables, fp32 / fp64 blends), then normalisation.  It is checked
          against the definition before it is timed.
Shapes: the 16-view ADE20K training batch (512 x 683 sources, short edge drawn from the config's sizes, crop 512 x 512,
ColorAugSSDTransform drawn per view) and the 16 LSJ views of tools/input_pipeline_bench.py at 1024 x 1024, with SSD
colour and with the video blends.

Times are host wall clock around calls that end in a device synchronise, routes alternated inside one process, median
and spread over the repetitions after a warm-up: the method of tools/input_pipeline_bench.py, whose ``measure`` this
tool calls.  No kernel-level time is taken.  A device is required.  Until this has been run on an MI355X and its output
committed under profiles/, no number exists for the colour stage.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bm2f_amd import (draw_color_aug_ssd, draw_video_photometric, image_views, lsj_view,  # noqa: E402
                      semantic_train_view)
from bm2f_amd import color_aug as ca  # noqa: E402
from input_pipeline_bench import MEAN, STD, measure  # noqa: E402

ADE_MIN_SIZES = tuple(int(x * 0.1 * 512) for x in range(5, 21))         # ade20k Base config: MIN_SIZE_TRAIN


# ------------------------------------------------------------------------------------------------ route (b)
def _convert_t(x, a, b):
    f = x.to(torch.float32) * torch.tensor(a, dtype=torch.float32, device=x.device)
    f = f + torch.tensor(b, dtype=torch.float32, device=x.device)
    return f.clamp(0, 255).to(torch.uint8)


def _bgr2hsv_t(p, sdiv, hdiv):
    p = p.to(torch.int32)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    v = torch.maximum(torch.maximum(b, g), r)
    diff = v - torch.minimum(torch.minimum(b, g), r)
    s = (diff * sdiv[v.long()] + 2048) >> 12
    h0 = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h0 * hdiv[diff.long()] + 2048) >> 12
    h = h + torch.where(h < 0, 180, 0)
    return torch.stack([h.clamp(0, 255), s, v], -1).to(torch.uint8)


def _hsv2bgr_t(p, sectors):
    one = torch.tensor(1.0, device=p.device)
    h = p[..., 0].float() * (torch.tensor(6.0) / torch.tensor(180.0)).to(p.device)
    s = p[..., 1].float() / 255.0
    v = p[..., 2].float() / 255.0
    sector = torch.floor(h)
    h = h - sector
    sector = sector.long()
    outside = (sector < 0) | (sector > 5)
    sector = torch.where(outside, 0, sector)
    h = torch.where(outside, 0.0, h)
    tab = torch.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1)
    bgr = torch.gather(tab, -1, sectors[sector])
    bgr = torch.where((p[..., 1] == 0)[..., None], v[..., None], bgr)
    return torch.round(bgr * 255.0).clamp(0, 255).to(torch.uint8)


def color_torch(px, aug, tabs):
    """The operations of ``aug`` on an (N, 3) uint8 device tensor of shown pixels, as tensor operations."""
    sdiv, hdiv, sectors = tabs
    x = px.flip(-1) if aug.swap_rb else px
    for name, val in aug.ops:
        if name in ("ssd_brightness", "ssd_contrast", "brightness"):
            a, b = {"ssd_brightness": (1.0, val), "ssd_contrast": (val, 0.0), "brightness": (val, (1 - val) * 0)}[name]
            x = _convert_t(x, a, b)
        elif name == "ssd_saturation":
            hsv = _bgr2hsv_t(x, sdiv, hdiv)
            hsv[..., 1] = _convert_t(hsv[..., 1], val, 0.0)
            x = _hsv2bgr_t(hsv, sectors)
        elif name == "ssd_hue":
            hsv = _bgr2hsv_t(x, sdiv, hdiv)
            hsv[..., 0] = ((hsv[..., 0].to(torch.int32) + int(val)) % 180).to(torch.uint8)
            x = _hsv2bgr_t(hsv, sectors)
        else:
            if name == "contrast":
                src = x.sum(dtype=torch.int64).double() / x.numel()
            else:       # torch has no fused multiply-add on fp64 tensors: this route is not held to the last bit
                src = (x.double() * torch.tensor(ca.GRAY_WEIGHTS, dtype=torch.float64, device=x.device)).sum(-1, True)
            y = (torch.tensor(val, dtype=torch.float32, device=x.device) * x.float()).double()
            x = ((1 - val) * src + y).clamp(0, 255).to(torch.uint8)
    return x.flip(-1) if aug.swap_rb else x


def routes_for(imgs, views, dev):
    mean_d = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_d = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    plain_views = [dataclasses.replace(v, color=None) for v in views]
    white = [torch.full(im.shape, 255, dtype=torch.uint8) for im in imgs]
    shown, _ = image_views(white, [dataclasses.replace(v, fill=0) for v in plain_views], out_dtype=torch.uint8)
    shown = (shown == 255).all(1).to(dev)                   # (V, Hp, Wp): geometry only, prepared outside the timing
    sdiv, hdiv = (torch.from_numpy(t).to(dev) for t in ca.hsv_tables())
    tabs = (sdiv, hdiv, torch.from_numpy(ca._SECTORS).to(dev))
    host_t = [torch.from_numpy(im) for im in imgs]

    def up():
        return [t.to(dev) for t in host_t]

    def fused():
        return image_views(up(), views, pixel_mean=MEAN, pixel_std=STD, out_dtype=torch.float32)[0]

    def plain():
        return image_views(up(), plain_views, pixel_mean=MEAN, pixel_std=STD, out_dtype=torch.float32)[0]

    def host():
        batch, _ = image_views(host_t, views, out_dtype=torch.uint8)
        return (batch.to(dev).float() - mean_d) / std_d

    def torch_u8():
        batch, _ = image_views(up(), plain_views, out_dtype=torch.uint8)
        for i, v in enumerate(views):
            if v.color is not None and v.color.ops:
                m = shown[i]
                px = batch[i].permute(1, 2, 0)[m]
                batch[i].permute(1, 2, 0)[m] = color_torch(px, v.color, tabs)
        return batch

    def torch_route():
        return (torch_u8().float() - mean_d) / std_d

    return {"fused": fused, "plain": plain, "host": host, "torch": torch_route}, torch_u8


def run_shape(name, imgs, views, dev, reps, result):
    routes, torch_u8 = routes_for(imgs, views, dev)
    want = routes["host"]()
    assert torch.equal(routes["fused"]().view(torch.int32), want.view(torch.int32)), name
    agree = torch.equal(routes["torch"]().view(torch.int32), want.view(torch.int32))
    r = measure(routes, reps)
    f, p, t = (r[k]["ms_median"] for k in ("fused", "plain", "torch"))
    result["shapes"][name] = {
        "views": len(views), "operations": [None if v.color is None else [list(o) for o in v.color.ops] for v in views],
        "routes": r, "colour_stage_ms_over_plain": f - p, "fused_over_torch": f / t,
        "fused_loses_to_torch": bool(f > t), "torch_route_equals_definition": bool(agree)}
    print(name, json.dumps(result["shapes"][name]["routes"]), "stage ms", f - p, "fused/torch", f / t, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_aug.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("color_aug_bench needs a HIP device: times from a CPU say nothing about it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "numpy": np.__version__, "torch": torch.__version__,
              "timing": "host wall clock around calls ending in a device synchronise; routes alternated; median over "
                        "the repetitions after a warm-up; no kernel-level time was taken",
              "exactness": "fused equals host (the numpy definition) bitwise, asserted before timing; torch is compared "
                           "and the outcome recorded per shape", "shapes": {}}
    imgs = [rng.integers(0, 256, (512, 683, 3), dtype=np.uint8) for _ in range(16)]
    views = [semantic_train_view(512, 683, min_sizes=ADE_MIN_SIZES, max_size=2048, crop_size=(512, 512), flip=True,
                                 color=True, rng=rng, size_divisibility=512, img_format="RGB", source=i)
             for i in range(16)]
    run_shape("ade20k_train_16_views_crop512_ssd", imgs, views, dev, a.reps, result)
    imgs = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(16)]
    params = [(float(rng.uniform(0.1, 2.0)), float(rng.uniform(0, 1)), bool(rng.integers(0, 2))) for _ in range(16)]
    lsj = [lsj_view(480, 640, 1024, s, o, f, source=i) for i, (s, o, f) in enumerate(params)]
    ssd = [dataclasses.replace(v, color=draw_color_aug_ssd(rng, img_format="RGB")) for v in lsj]
    run_shape("lsj_batch_16_at_1024_ssd", imgs, ssd, dev, a.reps, result)
    video = [dataclasses.replace(v, color=draw_video_photometric(rng, ["brightness", "contrast", "saturation"]))
             for v in lsj]
    run_shape("lsj_batch_16_at_1024_video_blends", imgs, video, dev, a.reps, result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
