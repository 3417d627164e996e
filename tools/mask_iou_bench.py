"""Time the device mask IoU (csrc/mask_iou.hip) against the only route to the same numbers without its kernels, on
the same machine, in the same run.

    python tools/mask_iou_bench.py [--dets 10] [--gts 5] [--frames 36] [--height 720] [--width 1280] [--reps 10]
                                   [--out profiles/mask_iou.json]

The workload is one YTVIS-like video: --dets detections and --gts ground truths of --frames frames, as `blobs`
(ellipses, a few runs per column) and as `speckle` (independent pixels at density 0.5, a run every two pixels: the
worst case of a run-length code; --speckle-frames frames, because the host route takes half a second per such mask).  Three routes, each checked for equal results before it is timed:

    decode     rle_to_bits of all (dets + gts) * frames masks on the device  vs  the host rle_decode of each
    pairs      mask_pair_counts on device planes                            vs  numpy `&` and `sum` on the decoded masks
    evaluate   evaluate_ytvis(device=cuda)                                   vs  host decode + numpy counts + the same
                                                                                 host matching (evaluate_ytvis on counts)

Times are wall milliseconds per call (host clock, a device synchronise before and after): the device route over
--reps calls after warm-up, the faster of two windows; the host route one call per window (two for blobs, one for
speckle); the string parsing, the upload and the copy back are part of the
device calls.  `kernel_ms` times the launches alone with device events; its bytes/s are the algorithmic bytes (every
input word read once, every output word written once) over that time, and `hbm_fraction` divides by the 8 TB/s
DESIGN.md uses.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import (YTVISGroundTruth, _native, evaluate_ytvis, mask_pair_counts, pack_mask_bits,  # noqa: E402
                      rle_decode, rle_encode, rle_to_bits)
from bm2f_amd.mask_iou import _run_ends, pair_tiles  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def both(device, host, reps, host_windows):
    """The host route is seconds of CPU work per call: one call per window, no warm-up."""
    td = min(timed(device, reps), timed(device, reps))
    th = min(timed(host, 1, warmup=0) for _ in range(host_windows))
    return {"device_ms": round(td, 4), "host_ms": round(th, 3), "host_over_device": round(th / td, 2)}


def kernel_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def masks_of(kind, n, T, H, W, g):
    if kind == "speckle":
        return torch.rand(n, T, H, W, generator=g) < 0.5
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(n, T, H, W, dtype=torch.bool)
    for i in range(n):
        cy, cx = torch.rand(2, generator=g) * torch.tensor([H, W]) * 0.6 + torch.tensor([H, W]) * 0.2
        ry, rx = torch.rand(2, generator=g) * torch.tensor([H, W]) * 0.25 + 20
        for t in range(T):
            out[i, t] = ((y - cy - 2 * t) / ry) ** 2 + ((x - cx - 3 * t) / rx) ** 2 <= 1
    return out


def host_counts(d_rles, g_rles, T):
    """The route without the kernels: rle_decode every mask, numpy `&` and `sum`."""
    d = np.stack([rle_decode(r).numpy() for r in d_rles]).reshape(-1, T, *d_rles[0]["size"])
    g = np.stack([rle_decode(r).numpy() for r in g_rles]).reshape(-1, T, *g_rles[0]["size"])
    inter = np.array([[(a & b).sum() for b in g] for a in d], dtype=np.int64)
    return inter, d.sum((2, 3)).astype(np.int64), g.sum((2, 3)).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=10)
    ap.add_argument("--gts", type=int, default=5)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--speckle-frames", type=int, default=2,
                    help="frames of the speckle video: its host route parses ~0.5 M runs per mask in Python")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_iou_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    D, G, H, W = a.dets, a.gts, a.height, a.width
    words = (W + 31) // 32
    ta, tb, chunk = pair_tiles()
    res = {"bench": "mask_iou", "device": torch.cuda.get_device_name(0), "dets": D, "gts": G, "frames": {"blobs": a.frames, "speckle": a.speckle_frames},
           "size": [H, W], "reps": a.reps, "tile": [ta, tb], "chunk_words": chunk}
    g = torch.Generator().manual_seed(0)
    for kind in ("blobs", "speckle"):
        T = a.frames if kind == "blobs" else a.speckle_frames
        dm, gm = masks_of(kind, D, T, H, W, g), masks_of(kind, G, T, H, W, g)
        d_rles, g_rles = rle_encode(dm.to(dev)), rle_encode(gm.to(dev))
        rles = d_rles + g_rles
        planes = rle_to_bits(rles, device=dev)
        if not torch.equal(planes.cpu(), pack_mask_bits(torch.cat([dm, gm]).flatten(0, 1))):
            raise SystemExit(f"mask_iou_bench: the decoded planes are wrong ({kind})")
        pa, pb = planes[:D * T].view(D, T, H, words), planes[D * T:].view(G, T, H, words)
        want = host_counts(d_rles, g_rles, T)
        if not all(np.array_equal(x, y) for x, y in zip(mask_pair_counts(pa, pb, W), want)):
            raise SystemExit(f"mask_iou_bench: the device and host counts disagree ({kind})")
        host_reps = 1 if kind == "speckle" else 2                      # windows of the host route
        r = {"rle_chars": sum(len(x["counts"]) for x in rles)}
        # decode
        r["decode"] = both(lambda: rle_to_bits(rles, device=dev), lambda: [rle_decode(x) for x in rles], a.reps,
                           host_reps)
        pos, off, _, _ = _run_ends(rles)
        dec_bytes = pos.size * 4 + off.size * 8 + planes.numel() * 4
        buf = torch.from_numpy(np.concatenate((off.view(np.int32), pos))).to(dev)
        off_d, pos_d = buf[:2 * off.size].view(torch.int64), buf[2 * off.size:]
        out = torch.empty_like(planes)
        st = torch.cuda.current_stream().cuda_stream
        k = kernel_ms(lambda: _native.call("m2f_rle_decode_bits", pos_d.data_ptr(), pos_d.numel(), off_d.data_ptr(),
                                           len(rles), H, W, out.data_ptr(), st), a.reps)
        r["decode"].update(kernel_ms=round(k, 4), algorithmic_bytes=dec_bytes,
                           bytes_per_s=round(dec_bytes / (k * 1e-3), 0),
                           hbm_fraction=round(dec_bytes / (k * 1e-3) / HBM_BYTES_PER_S, 4))
        # pairs
        r["pairs"] = both(lambda: mask_pair_counts(pa, pb, W), lambda: host_counts(d_rles, g_rles, T), a.reps,
                          host_reps)
        nbytes = ctypes.c_int64()
        _native.call("m2f_bits_pair_workspace", D, G, T, H, W, ctypes.byref(nbytes))
        work = torch.empty(nbytes.value // 4 + 1, dtype=torch.int32, device=dev)
        o = torch.empty(D * G + (D + G) * T, dtype=torch.int64, device=dev)
        n = T * H * words
        k = kernel_ms(lambda: _native.call("m2f_bits_pair_counts", pa.data_ptr(), D, n, pb.data_ptr(), G, n, T, H, W,
                                           o.data_ptr(), o[D * G:].data_ptr(), o[D * G + D * T:].data_ptr(),
                                           work.data_ptr(), work.numel() * 4, st), a.reps)
        pair_bytes = (D + G) * n * 4 + o.numel() * 8
        read_bytes = (D * -(-G // tb) + G * -(-D // ta)) * n * 4
        r["pairs"].update(kernel_ms=round(k, 4), algorithmic_bytes=pair_bytes, bytes_read_by_tiles=read_bytes,
                          bytes_per_s=round(pair_bytes / (k * 1e-3), 0),
                          hbm_fraction=round(pair_bytes / (k * 1e-3) / HBM_BYTES_PER_S, 4))
        # evaluate: one video, one category
        gt = YTVISGroundTruth({
            "videos": [{"id": 1, "height": H, "width": W, "length": T}], "categories": [{"id": 1, "name": "a"}],
            "annotations": [{"id": j + 1, "video_id": 1, "category_id": 1, "iscrowd": 0,
                             "segmentations": g_rles[j * T:(j + 1) * T], "areas": gm[j].sum((1, 2)).tolist()}
                            for j in range(G)]})
        results = [{"video_id": 1, "category_id": 1, "score": 1.0 - 0.05 * i,
                    "segmentations": d_rles[i * T:(i + 1) * T]} for i in range(D)]
        on_device = evaluate_ytvis(gt, results, device=dev)
        on_host = evaluate_ytvis(gt, results, _counts={1: host_counts(d_rles, g_rles, T)})
        if not (np.array_equal(on_device.precision, on_host.precision)
                and np.array_equal(on_device.ious[1, 1], on_host.ious[1, 1])):
            raise SystemExit(f"mask_iou_bench: the device and host evaluations disagree ({kind})")
        r["evaluate"] = both(lambda: evaluate_ytvis(gt, results, device=dev),
                             lambda: evaluate_ytvis(gt, results, _counts={1: host_counts(d_rles, g_rles, T)}),
                             a.reps, host_reps)
        r["evaluate"]["AP"] = round(float(on_device.stats[0]), 4)
        res[kind] = r
        del planes, pa, pb, out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
