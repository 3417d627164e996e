"""Time the polygon rasteriser (csrc/polygon.hip under bm2f_amd.polygon) on the device against the module's own numpy
host path, and the evaluator's batch step with polygon ground truth against the same batch with the ground truth
converted to RLE beforehand.

    python tools/polygon_bench.py [--reps 5] [--dets 20] [--out profiles/polygon_raster.json]

Two synthetic shapes:
    coco    48 images of 480 x 640, 7 annotations of one polygon of 40 vertices each
    large   8 images of 1024 x 2048, 4 annotations of 20 parts of 200 vertices each

    raster     polygons_to_bits_ragged(device=cuda)  vs  polygons_to_bits_ragged(device=cpu); the planes are
               compared word for word before anything is timed
    evaluator  coco_eval._segm_counts on --dets RLE detections per image with polygons="rasterize"  vs  the same
               with the ground truth from convert_polygons_to_rle (the conversion itself is timed separately)

Times are wall milliseconds per call (host clock, a device synchronise before and after), the faster of two windows
of --reps calls after a warm-up; the host-side table building, the upload and the copies are part of the device
route.  `host_tables_ms` is the share of `_plan` (checks, integer vertices, per-edge counts) alone.  No profiler trace
was taken.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import COCOGroundTruth, coco_eval, convert_polygons_to_rle, polygons_to_bits_ragged, rle_encode  # noqa: E402
from bm2f_amd import polygon  # noqa: E402

SHAPES = {"coco": dict(images=48, H=480, W=640, anns=7, parts=1, vertices=40),
          "large": dict(images=8, H=1024, W=2048, anns=4, parts=20, vertices=200)}


def timed(fn, reps, sync, warmup=1):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def best(fn, reps, sync=lambda: torch.cuda.synchronize()):
    return round(min(timed(fn, reps, sync) for _ in range(2)), 3)


def star(rng, H, W, vertices, scale):
    cx, cy = rng.uniform(0.25 * W, 0.75 * W), rng.uniform(0.25 * H, 0.75 * H)
    ang = np.sort(rng.uniform(0, 2 * np.pi, vertices))
    r = rng.uniform(0.4, 1.0, vertices) * scale * min(H, W)
    return np.stack((cx + r * np.cos(ang), cy + r * np.sin(ang)), 1).reshape(-1).round(2).tolist()


def dataset(images, H, W, anns, parts, vertices, dets, dev):
    rng = np.random.default_rng(0)
    ims, annotations, results = [], [], []
    for i in range(images):
        ims.append({"id": i + 1, "height": H, "width": W})
        segs = [[star(rng, H, W, vertices, 0.3 if parts == 1 else 0.15) for _ in range(parts)] for _ in range(anns)]
        for k, seg in enumerate(segs):
            annotations.append({"id": len(annotations) + 1, "image_id": i + 1, "category_id": 1 + k % 3, "iscrowd": 0,
                                "area": 1000.0, "segmentation": seg})
        det_segs = [[star(rng, H, W, vertices, 0.3)] for _ in range(dets)]
        words, off, _ = polygons_to_bits_ragged(det_segs, [(H, W)] * dets, device=dev)
        n = H * ((W + 31) // 32)
        planes = torch.stack([words[o:o + n].view(H, -1) for o in off])
        for k, rle in enumerate(rle_encode(planes, width=W)):
            results.append({"image_id": i + 1, "category_id": 1 + k % 3, "score": float(rng.uniform()),
                            "segmentation": rle})
    return {"images": ims, "annotations": annotations, "categories": [{"id": c, "name": str(c)} for c in (1, 2, 3)]}, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dets", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("polygon_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"bench": "polygon_raster", "device": torch.cuda.get_device_name(0), "reps": a.reps, "dets": a.dets}
    for name, shape in SHAPES.items():
        gt, results = dataset(dets=a.dets, dev=dev, **shape)
        segs = [x["segmentation"] for x in gt["annotations"]]
        sizes = [(shape["H"], shape["W"])] * len(segs)
        got = polygons_to_bits_ragged(segs, sizes, device=dev)
        want = polygons_to_bits_ragged(segs, sizes)
        n = shape["H"] * ((shape["W"] + 31) // 32)
        for o in got[1]:
            assert torch.equal(got[0][o:o + n].cpu(), want[0][o:o + n]), f"{name}: the planes differ"
        plan = polygon._plan(segs, np.asarray(sizes, dtype=np.int64))
        device_ms = best(lambda: polygons_to_bits_ragged(segs, sizes, device=dev), a.reps)
        host_ms = best(lambda: polygons_to_bits_ragged(segs, sizes), max(1, a.reps // 2), sync=lambda: None)
        tables_ms = best(lambda: polygon._plan(segs, np.asarray(sizes, dtype=np.int64)), a.reps, sync=lambda: None)
        # the evaluator's batch step
        convert_ms = best(lambda: convert_polygons_to_rle(gt, device=dev), max(1, a.reps // 2))
        gt_poly = COCOGroundTruth(gt, polygons="rasterize")
        gt_rle = COCOGroundTruth(convert_polygons_to_rle(gt, device=dev))
        img_ids = sorted(gt_poly.image_ids())
        dets_of = {}
        for r in results:
            dets_of.setdefault(r["image_id"], []).append(r)
        bb = coco_eval.DEFAULT_BATCH_BYTES
        c_poly = coco_eval._segm_counts(gt_poly, img_ids, dets_of, dev, bb)
        c_rle = coco_eval._segm_counts(gt_rle, img_ids, dets_of, dev, bb)
        for i in img_ids:
            assert all(np.array_equal(x, y) for x, y in zip(c_poly[i], c_rle[i])), f"{name}: image {i} differs"
        poly_ms = best(lambda: coco_eval._segm_counts(gt_poly, img_ids, dets_of, dev, bb), a.reps)
        rle_ms = best(lambda: coco_eval._segm_counts(gt_rle, img_ids, dets_of, dev, bb), a.reps)
        res[name] = {**shape, "annotations": len(segs), "polygons": plan.num_polys, "edges": int(plan.edges.shape[0]),
                     "crossings": plan.total, "plane_bytes": 4 * n * len(segs),
                     "raster": {"device_ms": device_ms, "numpy_host_ms": host_ms, "host_tables_ms": tables_ms,
                                "host_over_device": round(host_ms / device_ms, 2)},
                     "evaluator": {"batches": len(coco_eval.image_batches(gt_poly, img_ids, dets_of, bb)),
                                   "polygon_gt_ms": poly_ms, "converted_rle_gt_ms": rle_ms,
                                   "polygon_over_rle": round(poly_ms / rle_ms, 2),
                                   "convert_once_ms": convert_ms}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
