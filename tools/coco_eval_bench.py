"""Time the batched COCO mask counts (the ragged kernels of csrc/mask_iou.hip under evaluate_coco) against the route
that existed before them: a loop over the images with one rle_to_bits and one mask_pair_counts each.

    python tools/coco_eval_bench.py [--images 48] [--dets 100] [--gts 7] [--speckle-images 8] [--speckle-dets 10]
                                    [--reps 5] [--out profiles/coco_eval.json]

The set is synthetic: images of the sizes in SIZES in turn, --dets detections and --gts ground truths each, once as
`blobs` (ellipses, a few runs per column) and once as `speckle` (independent pixels at density 0.5, the worst case
of a run-length code; fewer images, the host parse of such a mask is long).  Both routes are checked for equal
counts before they are timed.

    counts     coco_eval._segm_counts (batches of --batch-bytes: one upload, one ragged decode, one ragged pair
               count, one copy per batch)        vs  per image: rle_to_bits + mask_pair_counts
    evaluate   evaluate_coco(device=cuda) as a whole (the counts plus the host matching both routes share)

Times are wall milliseconds per call (host clock, a device synchronise before and after), the faster of two windows
of --reps calls after a warm-up; parsing, uploads and copies are part of both routes.  `launches`, `uploads` and
`copies` are counted from the routes' structure (per batch: decode, pair, sum; per image: decode, pair, sum).
`launch_window_ms` puts device events around --kernel-reps back-to-back calls of the C entry points on the whole set as
one batch (buffers allocated once, no Python wrapper inside), divided by the calls: it holds the kernels' time plus
any gap the host leaves between enqueues, so it is an upper bound on kernel time, and the bytes/s from the
algorithmic bytes (every input word read once, every output word written once) and `hbm_fraction` (of the 8 TB/s
DESIGN.md uses) are lower bounds.  No profiler trace was taken.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import COCOGroundTruth, evaluate_coco, mask_pair_counts, rle_encode, rle_to_bits  # noqa: E402
from bm2f_amd import _native, coco_eval  # noqa: E402

mask_iou = importlib.import_module("bm2f_amd.mask_iou")            # the package also exports a function of that name

HBM_BYTES_PER_S = 8e12
SIZES = [(480, 640), (427, 640), (640, 480), (375, 500), (300, 200), (333, 500)]


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def launch_window_ms(fn, reps):
    """Device events around ``reps`` back-to-back calls, per call: kernel time plus whatever gap the host leaves
    between enqueues, so an upper bound on the kernels' own time."""
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def masks_of(kind, n, H, W, g, dev):
    if kind == "speckle":
        return (torch.rand(n, H, W, generator=g) < 0.5).to(dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    c = torch.rand(n, 4, generator=g).to(dev)
    cy, cx = (c[:, 0] * 0.6 + 0.2) * H, (c[:, 1] * 0.6 + 0.2) * W
    ry, rx = c[:, 2] * 0.25 * H + 8, c[:, 3] * 0.25 * W + 8
    return ((y - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((x - cx[:, None, None]) / rx[:, None, None]) ** 2 <= 1


def dataset(kind, images, dets, gts, dev):
    g = torch.Generator().manual_seed(0)
    ims, anns, results = [], [], []
    for i in range(images):
        H, W = SIZES[i % len(SIZES)]
        ims.append({"id": i + 1, "height": H, "width": W})
        m = masks_of(kind, dets + gts, H, W, g, dev)
        rles = rle_encode(m)
        areas = m.sum((1, 2)).tolist()
        for k in range(dets):
            results.append({"image_id": i + 1, "category_id": 1 + k % 3, "score": float(torch.rand(1, generator=g)),
                            "segmentation": rles[k]})
        for k in range(gts):
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": 1 + k % 3, "iscrowd": int(k == 6),
                         "area": float(areas[dets + k]), "segmentation": rles[dets + k]})
    gt = {"images": ims, "annotations": anns, "categories": [{"id": c, "name": str(c)} for c in (1, 2, 3)]}
    return COCOGroundTruth(gt), results


def loop_counts(gt, img_ids, dets_of, dev):
    """The route before the ragged kernels: per image one rle_to_bits and one mask_pair_counts."""
    out = {}
    for img_id in img_ids:
        dets, anns = dets_of.get(img_id, []), gt.img_to_anns.get(img_id, [])
        img = gt.imgs[img_id]
        H, W = img["height"], img["width"]
        coco_eval._check_segm(gt, img_id, dets, anns)                  # the batched route checks every mask too
        planes = rle_to_bits([r["segmentation"] for r in dets] + [a["segmentation"] for a in anns], device=dev,
                             size=(H, W))
        inter, aa, ab = mask_pair_counts(planes[:len(dets), None], planes[len(dets):, None], W)
        out[img_id] = (inter, aa.reshape(-1), ab.reshape(-1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=7)
    ap.add_argument("--speckle-images", type=int, default=8)
    ap.add_argument("--speckle-dets", type=int, default=10)
    ap.add_argument("--batch-bytes", type=int, default=coco_eval.DEFAULT_BATCH_BYTES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200, help="calls inside one device-event window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    ta, tb, chunk = mask_iou.pair_tiles()
    res = {"bench": "coco_eval", "device": torch.cuda.get_device_name(0), "sizes": SIZES, "gts": a.gts,
           "batch_bytes": a.batch_bytes, "reps": a.reps, "tile": [ta, tb], "chunk_words": chunk}
    for kind in ("blobs", "speckle"):
        images, dets = (a.images, a.dets) if kind == "blobs" else (a.speckle_images, a.speckle_dets)
        gt, results = dataset(kind, images, dets, a.gts, dev)
        img_ids = sorted(gt.image_ids())
        dets_of = {}
        for r in results:
            dets_of.setdefault(r["image_id"], []).append(r)
        batched = coco_eval._segm_counts(gt, img_ids, dets_of, dev, a.batch_bytes)
        looped = loop_counts(gt, img_ids, dets_of, dev)
        for i in img_ids:
            assert all(np.array_equal(x, y) for x, y in zip(batched[i], looped[i])), f"{kind}: image {i} differs"
        batches = len(coco_eval.image_batches(gt, img_ids, dets_of, a.batch_bytes))
        tb_ms = min(timed(lambda: coco_eval._segm_counts(gt, img_ids, dets_of, dev, a.batch_bytes), a.reps)
                    for _ in range(2))
        tl_ms = min(timed(lambda: loop_counts(gt, img_ids, dets_of, dev), a.reps) for _ in range(2))
        te_ms = min(timed(lambda: evaluate_coco(gt, results, device=dev, batch_bytes=a.batch_bytes), a.reps)
                    for _ in range(2))
        # the kernels alone, the whole set as one batch
        rles, groups = [], []
        for i in img_ids:
            n0, nd, ng = len(rles), len(dets_of[i]), len(gt.img_to_anns[i])
            rles += [r["segmentation"] for r in dets_of[i]] + [x["segmentation"] for x in gt.img_to_anns[i]]
            groups.append((gt.imgs[i]["height"], gt.imgs[i]["width"], np.arange(n0, n0 + nd),
                           np.arange(n0 + nd, n0 + nd + ng)))
        hw, offs, total, dtab = mask_iou._decode_plan(rles, None)
        desc, ptab, tiles = mask_iou._pair_plan([(H, W, offs[ia], offs[ib]) for H, W, ia, ib in groups], total)
        d = _native.upload_tables({**dtab, **ptab}, dev)
        words = torch.empty(total, dtype=torch.int32, device=dev)
        plane_words = int(mask_iou._plane_words(hw).sum())
        n_inter, n_a, n_b = int((desc[:, 2] * desc[:, 3]).sum()), int(desc[:, 2].sum()), int(desc[:, 3].sum())
        n_out = n_inter + n_a + n_b
        # the entry points themselves on buffers allocated once: no allocator and no Python wrapper inside the window
        nbytes = ctypes.c_int64()
        _native.call("m2f_bits_pair_ragged_workspace", tiles, ctypes.byref(nbytes))
        work = torch.empty(max(nbytes.value // 4, 1), dtype=torch.int32, device=dev)
        out = torch.empty(n_out, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        dec_args = (d["positions"].data_ptr(), d["positions"].numel(), d["offsets"].data_ptr(), len(rles),
                    d["sizes"].data_ptr(), d["out_offsets"].data_ptr(), d["blocks"].data_ptr(),
                    d["blocks"].numel() // 2, words.data_ptr(), words.numel(), st)
        pair_args = (words.data_ptr(), words.numel(), d["groups"].data_ptr(), desc.shape[0], d["a_off"].data_ptr(),
                     n_a, d["b_off"].data_ptr(), n_b, d["tiles"].data_ptr(), tiles, n_inter, out.data_ptr(),
                     out.data_ptr() + 8 * n_inter, out.data_ptr() + 8 * (n_inter + n_a), work.data_ptr(),
                     work.numel() * 4, st)
        kd = launch_window_ms(lambda: _native.call("m2f_rle_decode_bits_ragged", *dec_args), a.kernel_reps)
        kp = launch_window_ms(lambda: _native.call("m2f_bits_pair_counts_ragged", *pair_args), a.kernel_reps)
        dec_bytes = 4 * dtab["positions"].size + 16 * len(rles) + 4 * plane_words
        pair_bytes = 4 * plane_words + 8 * n_out

        def rate(nbytes, ms):
            return {"launch_window_ms": round(ms, 4), "window_reps": a.kernel_reps, "bytes": int(nbytes),
                    "tb_per_s_lower_bound": round(nbytes / ms / 1e9, 3),
                    "hbm_fraction_lower_bound": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}

        res[kind] = {
            "images": images, "dets": dets, "masks": len(rles), "rle_chars": sum(len(r["counts"]) for r in rles),
            "batches": batches, "pair_workgroups": int(tiles), "decode_workgroups": int(dtab["blocks"].shape[0]),
            "counts": {"batched_ms": round(tb_ms, 3), "per_image_loop_ms": round(tl_ms, 3),
                       "loop_over_batched": round(tl_ms / tb_ms, 2)},
            "evaluate_coco_ms": round(te_ms, 3),
            "batched": {"launches": 3 * batches, "uploads": batches, "copies": batches},
            "per_image_loop": {"launches": 3 * images, "uploads": images, "copies": images},
            "decode": rate(dec_bytes, kd), "pairs": rate(pair_bytes, kp)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
