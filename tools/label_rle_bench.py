"""Time label_maps_to_rle and rle_to_label_maps against the best routes to the same results without them, on the same
GPU, in the same run.

    python tools/label_rle_bench.py [--reps 7] [--out profiles/label_rle.json]

Shapes
    semantic   16 uint8 maps of 512 x 683, about 10 of 150 classes present each (regions of 32 x 32 pixels)
    panoptic   16 int32 maps of 800 x 1216 with about 40 segments each (ids as rgb2id gives them), encoded in the
               order of a segments_info (``ids=``)
    random     one uint8 map of 512 x 683 with a label drawn per pixel from 150: the worst case, one run per pixel,
               so the sort has H * W keys

Encoder: `new` is one label_maps_to_rle call over the batch.  `baseline` is, per image, one broadcast ``==`` of the map
against its values into (S, H, W) uint8 masks on the device and one rle_encode of them; the values are the image's
``torch.unique`` (semantic, random) or the given ids (panoptic).  The baseline computes no area and no box.  The two
routes must return equal strings, or the tool fails.
Painter: `new` is one rle_to_label_maps call over the batch's segments.  `baseline` is rle_to_bits_ragged of all
segments, then per segment the bit plane unpacked with torch and ``plane[mask] = value``.  Equal planes, or the tool
fails.

Each time is wall milliseconds per call (host clock, a device synchronise before and after each call), the median of
--reps calls per route, the two routes alternated call by call, after two warm-up calls of each.  `d2h_bytes` counts
what Tensor.cpu() moved from the device in one call, `peak_bytes` the rise of torch.cuda.max_memory_allocated over one
call.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import label_maps_to_rle, rle_encode, rle_to_bits_ragged, rle_to_label_maps  # noqa: E402
from tools.rle_bench import d2h_bytes, peak  # noqa: E402


def one_call(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(new, baseline, reps):
    for _ in range(2):
        new()
        baseline()
    tn, tb = [], []
    for _ in range(reps):
        tn.append(one_call(new))
        tb.append(one_call(baseline))
    n, b = statistics.median(tn), statistics.median(tb)
    return {"new_ms": round(n, 3), "baseline_ms": round(b, 3), "baseline_over_new": round(b / n, 2),
            "new_d2h_bytes": d2h_bytes(new), "baseline_d2h_bytes": d2h_bytes(baseline),
            "new_peak_bytes": peak(new), "baseline_peak_bytes": peak(baseline)}


def regions(h, w, cell, values, g):
    """A map of cell x cell regions, each holding one of `values`."""
    low = values[torch.randint(0, len(values), ((h + cell - 1) // cell, (w + cell - 1) // cell), generator=g)]
    return low.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:h, :w].contiguous()


def unpack(words, off, H, W):
    rows = words[off:off + H * ((W + 31) // 32)].view(H, -1)
    bits = (rows[:, :, None] >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1
    return bits.view(H, -1)[:, :W].bool()


def bench_shape(planes, ids, reps):
    """planes on the device; ids None (every value present) or the per-image lists."""
    dev = planes[0].device

    def enc_new():
        return label_maps_to_rle(planes, ids=ids)

    def enc_baseline():
        out = []
        for i, p in enumerate(planes):
            values = torch.unique(p) if ids is None else torch.tensor(ids[i], dtype=p.dtype, device=dev)
            out.append(rle_encode((p[None] == values[:, None, None]).to(torch.uint8)))
        return out

    got, want = enc_new(), enc_baseline()
    if [[e["segmentation"] for e in one] for one in got] != want:
        raise SystemExit("label_rle_bench: the encoder routes disagree")
    segments = [[(e["label"], e["segmentation"]) for e in one] for one in got]
    sizes = [tuple(p.shape) for p in planes]
    flat = [(i, v, r) for i, one in enumerate(segments) for v, r in one]

    def paint_new():
        return rle_to_label_maps(segments, sizes, fill=0, dtype=planes[0].dtype, device=dev)

    def paint_baseline():
        words, offsets, hw = rle_to_bits_ragged([r for _, _, r in flat], device=dev)
        out = [torch.zeros(s, dtype=planes[0].dtype, device=dev) for s in sizes]
        for (i, v, _), off, (H, W) in zip(flat, offsets.tolist(), hw.tolist()):
            out[i][unpack(words, off, H, W)] = v
        return out

    for a, b, p in zip(paint_new(), paint_baseline(), planes):
        if not (torch.equal(a, b) and torch.equal(a, p)):
            raise SystemExit("label_rle_bench: the painter routes disagree")
    return {"images": len(planes), "size": list(sizes[0]), "dtype": str(planes[0].dtype).replace("torch.", ""),
            "segments": len(flat), "encoded_bytes": sum(len(r["counts"]) for _, _, r in flat),
            "encode": compare(enc_new, enc_baseline, reps), "paint": compare(paint_new, paint_baseline, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_rle_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"bench": "label_rle", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    sem = [regions(512, 683, 32, torch.randperm(150, generator=g)[:10], g).to(torch.uint8).to(dev) for _ in range(16)]
    res["semantic"] = bench_shape(sem, None, a.reps)
    pan, pan_ids = [], []
    for _ in range(16):
        values = torch.randint(1, 2 ** 24, (40,), generator=g)
        m = regions(800, 1216, 64, values, g)
        pan.append(m.to(torch.int32).to(dev))
        present = set(torch.unique(m).tolist())
        pan_ids.append([v for v in dict.fromkeys(values.tolist()) if v in present])     # segments_info order
    res["panoptic"] = bench_shape(pan, pan_ids, a.reps)
    rnd = [torch.randint(0, 150, (512, 683), generator=g).to(torch.uint8).to(dev)]
    res["random"] = bench_shape(rnd, None, max(3, a.reps // 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
