"""Time instance_views (csrc/bits_views.hip) against the best route without it at the same commit, and write
profiles/instance_views.json.

    python tools/instance_views_bench.py [--reps N] [--out profiles/instance_views.json]

Both routes start from planes that are on the device already and end with uint8 masks, float boxes and areas:

  new     the packed bit planes of rle_to_bits_ragged -> one instance_views call for the batch (one table upload, two
          launches, no device-to-host copy)
  dense   the same masks unpacked to one byte per pixel -> one label_views(seg_pad=0) call per image (its P differs),
          then BitMasks.get_bounding_boxes as batched torch operations (any, argmax of the flags and of their mirror,
          sum), which need no synchronisation

Decoding the annotations is outside both (the dense route would pay an unpack on top).  Shapes: a COCO-LSJ-like batch,
16 images of 480 x 640 with 1-20 instances each mapped to 1024 x 1024; a YouTube-VIS-like batch, 8 clips of 2 frames of
360 x 640.  Timing: host wall clock around calls ending in a device synchronise, routes alternated, median over the
repetitions after a warm-up; one run; no kernel-level time and no counters were taken.  The launch and copy counts are
read off the code, not traced.  The tool asserts that both routes give equal masks, boxes and areas before it times.
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

from bm2f_amd import instance_views, label_views, lsj_view, video_clip_views  # noqa: E402
from bm2f_amd.video_inference import pack_mask_bits  # noqa: E402
from input_pipeline_bench import measure  # noqa: E402

YTVIS_MIN_SIZES = (288, 320, 352, 392, 416, 448, 480, 512)             # youtubevis_2019 Base config


def blobs(rng, n, hw):
    """n masks of an (H, W) image: a few rectangles each, as instance masks go."""
    H, W = hw
    out = np.zeros((n, H, W), dtype=np.uint8)
    for m in out:
        for _ in range(int(rng.integers(1, 4))):
            h, w = int(rng.integers(8, H // 2)), int(rng.integers(8, W // 2))
            y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            m[y:y + h, x:x + w] = 1
    return out


def boxes_torch(m):
    """BitMasks.get_bounding_boxes and the area of (G, H, W) uint8 masks, batched, without a synchronisation."""
    xa, ya = m.any(1), m.any(2)
    W, H = xa.shape[1], ya.shape[1]
    x0, y0 = xa.int().argmax(1), ya.int().argmax(1)
    x1, y1 = W - xa.flip(1).int().argmax(1), H - ya.flip(1).int().argmax(1)
    some = xa.any(1)
    box = torch.stack((x0, y0, x1, y1), 1) * some[:, None]
    return box.float(), m.sum((1, 2), dtype=torch.int32)


def run_shape(name, masks, views, dev, reps, result):
    dense_d = [torch.from_numpy(m).to(dev) for m in masks]
    bits = [pack_mask_bits(d.bool()).reshape(-1) for d in dense_d]
    words = torch.cat(bits)
    sizes = np.array([m.shape[1:] for m in masks for _ in m], dtype=np.int64)
    per = sizes[:, 0] * ((sizes[:, 1] + 31) // 32)
    offsets = np.concatenate(([0], np.cumsum(per)))[:-1]
    view_of = np.array([i for i, m in enumerate(masks) for _ in m], dtype=np.int64)

    def new():
        return instance_views(words, offsets, sizes, view_of, views, out="uint8")[:3]

    def dense():
        out = []
        for i, d in enumerate(dense_d):
            m = label_views([d], [dataclasses.replace(views[i], source=0, color=None)], seg_pad=0)[0][0]
            out.append((m,) + boxes_torch(m))
        return out

    got, want = new(), dense()
    at = 0
    for m, b, s in want:
        rows = slice(at, at + m.shape[0])
        assert torch.equal(got[0][rows, :m.shape[1], :m.shape[2]], m), name
        assert int(got[0][rows].sum()) == int(s.sum()), name              # nothing beyond the view's canvas
        assert torch.equal(got[1][rows], b) and torch.equal(got[2][rows], s), name
        at += m.shape[0]
    r = measure({"new": new, "dense": dense}, reps)
    n, d = r["new"]["ms_median"], r["dense"]["ms_median"]
    result["shapes"][name] = {
        "images": len(masks), "instances": int(view_of.size), "routes": r, "new_over_dense": n / d,
        "new_loses_to_dense": bool(n > d),
        "new_counts": {"launches": 2, "host_to_device_copies": 1, "device_to_host_copies": 0},
        "dense_counts": {"label_views_launches": len(masks), "host_to_device_copies": len(masks),
                         "device_to_host_copies": 0, "torch_operations": "about 14 per image, not traced"},
        "input_bytes": {"new": int(words.numel() * 4), "dense": int(sum(d.numel() for d in dense_d))}}
    print(name, json.dumps(result["shapes"][name]), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_views.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("instance_views_bench needs a HIP device: times from a CPU say nothing about it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "numpy": np.__version__, "torch": torch.__version__,
              "timing": "host wall clock around calls ending in a device synchronise; routes alternated; median over "
                        "the repetitions after a warm-up; one run; no kernel-level time and no counters were taken; "
                        "launch and copy counts are read off the code",
              "exactness": "both routes give equal masks, boxes and areas, asserted before timing", "shapes": {}}
    counts = [int(rng.integers(1, 21)) for _ in range(16)]
    masks = [blobs(rng, n, (480, 640)) for n in counts]
    views = [lsj_view(480, 640, 1024, float(rng.uniform(0.1, 2.0)), float(rng.uniform(0, 1)), bool(rng.integers(0, 2)),
                      source=i) for i in range(16)]
    run_shape("coco_lsj_16_images_1_to_20_instances_at_1024", masks, views, dev, a.reps, result)
    masks, views = [], []
    for _ in range(8):
        n = int(rng.integers(1, 7))
        masks += [blobs(rng, n, (360, 640)) for _ in range(2)]
        views += video_clip_views([(360, 640)] * 2, min_sizes=YTVIS_MIN_SIZES, max_size=768,
                                  sample_style="choice_by_clip", random_flip="flip_by_clip", augmentations=(),
                                  clip_frame_cnt=2, rng=rng)
    views = [dataclasses.replace(v, source=i) for i, v in enumerate(views)]
    run_shape("ytvis_8_clips_of_2_frames_360x640", masks, views, dev, a.reps, result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
