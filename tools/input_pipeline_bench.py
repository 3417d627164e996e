"""Wall time, peak device memory and uploaded bytes of the device input pipeline (bm2f_amd/image_views.py) against
two baselines, written to profiles/input_pipeline.json.

    python tools/input_pipeline_bench.py [--reps N] [--out profiles/input_pipeline.json]

Routes, all ending with the views on the device after a synchronise:
  new    one upload of the uint8 source(s), one m2f_image_views launch (PIL-exact);
  pil    the reference's route: Pillow resize per view on the host, upload per view, then torch flip / normalise /
         pad / stack on the device (PIL-exact by definition; skipped, "not measured", where Pillow is missing);
  torch  the best device route without this module: upload, F.interpolate(antialias=True) per view, flip,
         normalise, pad and stack.  This route is NOT PIL-exact: it is a speed baseline only.
Shapes: the 12 ADE20K TTA views of a 512 x 683 image, the 12 Cityscapes TTA views of a 1024 x 2048 image (up to
1792 x 3584), and a batch of 16 LSJ training views at 1024 x 1024 from 480 x 640 sources.

Times are host wall clock around calls that end in a device synchronise, routes alternated inside one process, median
and spread over the repetitions after a warm-up.  No kernel-level time is taken (no profiler run).  A device is
required: there is no CPU timing.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bm2f_amd import View, image_views, lsj_view, tta_view_sizes  # noqa: E402

MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def tta_routes(img, sizes, dev):
    """img: uint8 (H, W, 3) numpy.  Every route returns the V uint8 / float (3, h, w) views on the device."""
    Image = _pil()
    views = [View(size=(h, w), flip_out=f) for h, w, f in sizes]
    host = torch.from_numpy(img)

    def new():
        batch, _ = image_views([host.to(dev)], views, out_dtype=torch.uint8)
        return batch

    def pil():
        out, pim = [], Image.fromarray(img)
        for h, w, f in sizes:
            a = np.asarray(pim.resize((w, h), Image.BILINEAR))
            a = a[:, ::-1] if f else a
            out.append(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dev))
        return out

    def torch_route():
        x = host.to(dev).permute(2, 0, 1)[None].float()
        out = []
        for h, w, f in sizes:
            v = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False, antialias=True)[0]
            out.append(v.flip(-1) if f else v)
        return out

    uploads = {"new": img.nbytes, "pil": sum(3 * h * w for h, w, _ in sizes), "torch": img.nbytes}
    return {"new": new, "pil": pil if Image else None, "torch": torch_route}, uploads


def lsj_routes(imgs, params, S, dev):
    """imgs: uint8 (H, W, 3) numpy sources; params: (scale, offset_frac, flip) per image; fp32 normalised (B, 3, S, S)."""
    Image = _pil()
    views = [lsj_view(*im.shape[:2], S, s, o, f, source=i) for i, (im, (s, o, f)) in enumerate(zip(imgs, params))]
    mean = torch.tensor(MEAN, device=dev).view(3, 1, 1)
    std = torch.tensor(STD, device=dev).view(3, 1, 1)

    def new():
        batch, _ = image_views([torch.from_numpy(im).to(dev) for im in imgs], views, pixel_mean=MEAN, pixel_std=STD,
                               out_dtype=torch.float32)
        return batch

    def place(x, v):                                        # (3, rh, rw) on the device -> (3, S, S), fill 128
        y0, x0 = v.crop[:2]
        x = x[:, y0:y0 + S, x0:x0 + S]
        return F.pad(x, (0, S - x.shape[2], 0, S - x.shape[1]), value=128)

    def pil():
        out = []
        for im, v in zip(imgs, views):
            a = im[:, ::-1] if v.flip_in else im
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((v.size[1], v.size[0]), Image.BILINEAR))
            y0, x0 = v.crop[:2]
            a = np.ascontiguousarray(a[y0:y0 + S, x0:x0 + S].transpose(2, 0, 1))
            x = torch.from_numpy(a).to(dev)
            x = F.pad(x, (0, S - x.shape[2], 0, S - x.shape[1]), value=128)
            out.append((x.float() - mean) / std)
        return torch.stack(out)

    def torch_route():
        out = []
        for im, v in zip(imgs, views):
            x = torch.from_numpy(im).to(dev).permute(2, 0, 1)[None].float()
            x = x.flip(-1) if v.flip_in else x
            x = F.interpolate(x, size=v.size, mode="bilinear", align_corners=False, antialias=True)[0]
            out.append((place(x, v) - mean) / std)
        return torch.stack(out)

    up_new = sum(im.nbytes for im in imgs)
    up_pil = sum(3 * min(S, v.size[0] - v.crop[0]) * min(S, v.size[1] - v.crop[1]) for v in views)
    return {"new": new, "pil": pil if Image else None, "torch": torch_route}, {"new": up_new, "pil": up_pil,
                                                                              "torch": up_new}


def measure(routes, reps, warmup=2):
    names = [n for n, f in routes.items() if f is not None]
    times = {n: [] for n in names}
    peak = {}
    for n in names:
        for _ in range(warmup):
            routes[n]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = routes[n]()
        torch.cuda.synchronize()
        peak[n] = torch.cuda.max_memory_allocated() - base
        del r
    for _ in range(reps):                                   # alternate the routes: drift hits them alike
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = routes[n]()
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
            del r
    out = {}
    for n, f in routes.items():
        if f is None:
            out[n] = "not measured (Pillow is not installed on the measuring machine)"
        else:
            t = sorted(times[n])
            out[n] = {"ms_median": statistics.median(t) * 1e3, "ms_min": t[0] * 1e3, "ms_max": t[-1] * 1e3,
                      "reps": len(t), "peak_device_bytes": int(peak[n])}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pipeline.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("input_pipeline_bench needs a HIP device: times from a CPU say nothing about it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    Image = _pil()
    result = {"device": torch.cuda.get_device_name(0), "pillow": getattr(sys.modules.get("PIL"), "__version__", None),
              "timing": "host wall clock around calls ending in a device synchronise; routes alternated; no kernel-"
                        "level time was taken", "exactness": "new and pil are PIL-exact; torch is not", "shapes": {}}
    shapes = {"ade20k_tta_12_views_512x683": ((512, 683), (256, 384, 512, 640, 768, 896), 3584),
              "cityscapes_tta_12_views_1024x2048": ((1024, 2048), (512, 768, 1024, 1280, 1536, 1792), 4096)}
    for name, ((H, W), min_sizes, max_size) in shapes.items():
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        sizes = tta_view_sizes(H, W, min_sizes, max_size, True)
        routes, uploads = tta_routes(img, sizes, dev)
        if Image:                                           # the timed routes agree where they must
            got, want = routes["new"](), routes["pil"]()
            assert all(torch.equal(got[i, :, :h, :w], want[i]) for i, (h, w, _) in enumerate(sizes)), name
        r = measure(routes, a.reps)
        result["shapes"][name] = {"views": [list(s) for s in sizes], "uploaded_bytes": uploads, "routes": r}
        print(name, json.dumps(r), flush=True)
    imgs = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(16)]
    params = [(float(rng.uniform(0.1, 2.0)), float(rng.uniform(0, 1)), bool(rng.integers(0, 2))) for _ in range(16)]
    routes, uploads = lsj_routes(imgs, params, 1024, dev)
    if Image:
        assert torch.equal(routes["new"]().view(torch.int32), routes["pil"]().view(torch.int32)), "lsj"
    r = measure(routes, a.reps)
    result["shapes"]["lsj_batch_16_at_1024_from_480x640"] = {"params": params, "uploaded_bytes": uploads, "routes": r}
    print("lsj", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
