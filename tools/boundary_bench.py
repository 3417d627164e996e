"""Time the device boundary kernel (csrc/mask_boundary.hip) and Boundary AP against two routes to the same planes
that share none of its code, on the same machine, in the same run.

    python tools/boundary_bench.py [--images 48] [--dets 100] [--gts 7] [--speckle-images 8] [--speckle-dets 10]
                                   [--reps 5] [--out profiles/boundary_iou.json]

The workload is that of tools/coco_eval_bench.py: images of its SIZES in turn (about 480 x 640, d = 7 .. 16 at the
default ratio), --dets detections and --gts ground truths each, as `blobs` and as `speckle` (independent pixels at
density 0.5).  Every route is checked for equal planes before it is timed.

    boundary   boundary_bits_ragged on the whole set's planes in one buffer (one upload of the table, one launch)
        vs host    rle_decode + scipy.ndimage.binary_erosion(3 x 3, d iterations) per mask, timed on --host-masks
                   masks and scaled to the set (marked `scaled`)
        vs dense   dense device masks of one image at a time, zero-padded by d and eroded by
                   -max_pool2d(-x, 2d + 1, stride 1), timed on --dense-images images and scaled to the set
    evaluate   evaluate_coco(iou_type="boundary", device=cuda)  vs  evaluate_coco(iou_type="segm", device=cuda), the
               parent code path, unchanged by this kernel

Wall times are milliseconds per call (host clock, a device synchronise before and after), the faster of two windows
of --reps calls after a warm-up.  `launch_window_ms` puts device events around --kernel-reps back-to-back calls of the
C entry point on buffers allocated once: kernel time plus any gap the host leaves between enqueues, so an upper bound
on kernel time; the bytes/s from the algorithmic bytes (every plane word read once and written once) and
`hbm_fraction` (of the 8 TB/s DESIGN.md uses) are lower bounds.  `fits_infinity_cache` says whether both buffers
together are below the 256 MiB last-level cache, in which case the repeated launches of the window are served from
it and the rate is not an HBM rate.  No profiler trace was taken.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bm2f_amd import (_native, boundary_bits_ragged, boundary_dilation, evaluate_coco, rle_decode,  # noqa: E402
                      rle_to_bits_ragged, unpack_mask_bits)
from coco_eval_bench import HBM_BYTES_PER_S, SIZES, dataset, launch_window_ms, timed  # noqa: E402

mb = importlib.import_module("bm2f_amd.mask_boundary")
INFINITY_CACHE_BYTES = 256 << 20


def host_boundary(rle, d):
    m = rle_decode(rle).numpy().astype(bool)
    return m & ~ndimage.binary_erosion(m, structure=np.ones((3, 3), dtype=bool), iterations=d, border_value=0)


def dense_boundary(x, d):
    """x (N, H, W) float on the device, 0 / 1 -> bool boundary; outside the image counts as zero."""
    padded = F.pad(x[:, None], (d, d, d, d))
    eroded = -F.max_pool2d(-padded, 2 * d + 1, 1)
    return (x > 0) & ~(eroded[:, 0] > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=7)
    ap.add_argument("--speckle-images", type=int, default=8)
    ap.add_argument("--speckle-dets", type=int, default=10)
    ap.add_argument("--host-masks", type=int, default=24)
    ap.add_argument("--dense-images", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=100, help="calls inside one device-event window")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench: needs a HIP device")
    dev = torch.device(a.device)
    band, tile_words, d_max = mb.boundary_tiles()
    res = {"bench": "boundary_iou", "device": torch.cuda.get_device_name(0), "sizes": SIZES, "gts": a.gts,
           "dilation_ratio": 0.02, "reps": a.reps, "band_rows": band, "tile_words": tile_words, "d_max": d_max}
    for kind in ("blobs", "speckle"):
        images, dets = (a.images, a.dets) if kind == "blobs" else (a.speckle_images, a.speckle_dets)
        gt, results = dataset(kind, images, dets, a.gts, dev)
        img_ids = sorted(gt.image_ids())
        dets_of = {}
        for r in results:
            dets_of.setdefault(r["image_id"], []).append(r)
        rles, per_image = [], []
        for i in img_ids:
            n0 = len(rles)
            rles += [r["segmentation"] for r in dets_of[i]] + [x["segmentation"] for x in gt.img_to_anns[i]]
            per_image.append((n0, len(rles)))
        words, offsets, hw = rle_to_bits_ragged(rles, device=dev)
        d = np.array([boundary_dilation(H, W) for H, W in hw])
        edges = boundary_bits_ragged(words, offsets, hw)
        host_edges = edges.cpu().numpy()

        def plane(m):
            H, W = hw[m]
            return host_edges[offsets[m]:offsets[m] + H * ((W + 31) // 32)].reshape(H, -1)

        # the two baselines give the kernel's planes
        step = max(1, len(rles) // a.host_masks)
        host_set = list(range(0, len(rles), step))[:a.host_masks]
        for m in host_set:
            want = mb._pack_rows(host_boundary(rles[m], int(d[m])))
            assert np.array_equal(plane(m), want), f"{kind}: mask {m} differs from the scipy route"
        dense_set = list(range(min(a.dense_images, len(img_ids))))
        dense_in = []
        for k in dense_set:
            n0, n1 = per_image[k]
            H, W = hw[n0]
            stack = torch.stack([words[offsets[m]:offsets[m] + H * ((W + 31) // 32)].view(H, -1)
                                 for m in range(n0, n1)])
            x = unpack_mask_bits(stack, int(W)).to(torch.float16)
            dense_in.append((x, int(d[n0])))
            got = dense_boundary(x, int(d[n0])).cpu().numpy()
            for j, m in enumerate(range(n0, n1)):
                assert np.array_equal(mb._pack_rows(got[j]), plane(m)), f"{kind}: mask {m} differs from max_pool2d"

        plane_words = int((hw[:, 0] * ((hw[:, 1] + 31) // 32)).sum())
        t_dev = min(timed(lambda: boundary_bits_ragged(words, offsets, hw), a.reps) for _ in range(2))
        t_host = min(timed(lambda: [host_boundary(rles[m], int(d[m])) for m in host_set], 1, warmup=0)
                     for _ in range(2)) * len(rles) / len(host_set)
        t_dense = min(timed(lambda: [dense_boundary(x, dd) for x, dd in dense_in], 1) for _ in range(2)) \
            * len(img_ids) / len(dense_set)
        t_bd = min(timed(lambda: evaluate_coco(gt, results, iou_type="boundary", device=dev), a.reps) for _ in range(2))
        t_sg = min(timed(lambda: evaluate_coco(gt, results, iou_type="segm", device=dev), a.reps) for _ in range(2))

        # the entry point alone on buffers allocated once
        tables, num_blocks = mb._boundary_plan(hw, offsets, d, words.numel())
        t = _native.upload_tables(tables, dev)
        out = torch.empty_like(words)
        st = torch.cuda.current_stream(dev).cuda_stream
        args = (words.data_ptr(), words.numel(), len(rles), t["bd_sizes"].data_ptr(), t["bd_offsets"].data_ptr(),
                t["bd_dilations"].data_ptr(), t["bd_blocks"].data_ptr(), num_blocks, int(d.max()), out.data_ptr(), st)
        k_ms = min(launch_window_ms(lambda: _native.call("m2f_bits_boundary_ragged", *args), a.kernel_reps)
                   for _ in range(2))
        assert all(torch.equal(out[o:o + H * ((W + 31) // 32)], edges[o:o + H * ((W + 31) // 32)])
                   for o, (H, W) in zip(offsets, hw)), f"{kind}: the timed launches give other planes"
        nbytes = 8 * plane_words
        res[kind] = {
            "images": images, "dets": dets, "masks": len(rles), "plane_bytes": 4 * plane_words,
            "dilations": sorted(set(int(v) for v in d)), "workgroups": int(num_blocks),
            "boundary": {"device_ms": round(t_dev, 3),
                         "host_scipy_ms_scaled": round(t_host, 1), "host_masks_timed": len(host_set),
                         "dense_max_pool2d_ms_scaled": round(t_dense, 2), "dense_images_timed": len(dense_set),
                         "host_over_device": round(t_host / t_dev, 1), "dense_over_device": round(t_dense / t_dev, 2)},
            "evaluate": {"boundary_ms": round(t_bd, 2), "segm_ms": round(t_sg, 2),
                         "boundary_over_segm": round(t_bd / t_sg, 3)},
            "kernel": {"launch_window_ms": round(k_ms, 4), "window_reps": a.kernel_reps, "bytes": int(nbytes),
                       "tb_per_s_lower_bound": round(nbytes / k_ms / 1e9, 3),
                       "hbm_fraction_lower_bound": round(nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4),
                       "fits_infinity_cache": bool(nbytes < INFINITY_CACHE_BYTES)}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
