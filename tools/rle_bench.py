"""Time the heads' device RLE encoding against the fastest route to the same result without the RLE kernels, on the
same GPU, in the same run.

    python tools/rle_bench.py [--frames 8] [--height 480] [--width 640] [--image 1024] [--reps 10]
                              [--out profiles/rle_results.json]

Video: Q = 100, K = 40, one clip of --frames frames padded to --height x --width (image 8 pixels smaller each way,
output the padded size), logits at a quarter of the padded size, fp32 and fp16.  `device` is
VideoMaskFormerInference(rle=True); `host` is the packed=True head followed by the host definition of rle_encode on
the packed words.  Both are run on two kinds of logits: `noise` (independent normal values at the logits'
resolution, which upsample to speckle with a run every few pixels: the worst case for a run-length code) and `blobs`
(the same at an eighth of that resolution, upsampled: connected regions, a few runs per column).  Image: B = 1,
Q = 100, 100 detections at --image squared from logits at a quarter of it, fp32, the same two kinds.  `device` is MaskFormerInference(instance_rle=True); `host` is the default head, `pred_masks > 0` copied to the
host as bool, and the host rle_encode.  The two routes must return equal results, or the tool fails.

Each time is wall milliseconds per call (host clock, a device synchronise before and after) over --reps calls after
warm-up, the faster of two alternated windows; the host's encoding is CPU work and is part of the call.
`d2h_bytes` counts what Tensor.cpu() moved from the device in one call, `peak_bytes` the rise of
torch.cuda.max_memory_allocated over one call.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import MaskFormerInference, VideoMaskFormerInference, rle_encode  # noqa: E402

Q, K, TOPK = 100, 40, 10


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del r
    return int(p)


def d2h_bytes(fn):
    """Bytes Tensor.cpu() moves from the device during one call."""
    moved = [0]
    orig = torch.Tensor.cpu

    def counting(t, *a, **kw):
        if t.device.type == "cuda":
            moved[0] += t.numel() * t.element_size()
        return orig(t, *a, **kw)

    torch.Tensor.cpu = counting
    try:
        fn()
    finally:
        torch.Tensor.cpu = orig
    return moved[0]


def both(device, host, reps):
    t = [timed(device, reps), timed(host, reps), timed(device, reps), timed(host, reps)]
    td, th = min(t[0], t[2]), min(t[1], t[3])
    return {"device_ms": round(td, 4), "host_ms": round(th, 4), "host_over_device": round(th / td, 2),
            "device_d2h_bytes": d2h_bytes(device), "host_d2h_bytes": d2h_bytes(host),
            "device_peak_bytes": peak(device), "host_peak_bytes": peak(host)}


def logits(shape, kind, g):
    """(..., h, w) normal logits; `blobs` draws them at an eighth of the resolution and upsamples."""
    if kind == "noise":
        return torch.randn(*shape, generator=g) * 3
    lead, (h, w) = shape[:-2], shape[-2:]
    low = torch.randn(*lead, max(h // 8, 2), max(w // 8, 2), generator=g) * 3
    return F.interpolate(low.flatten(0, -3)[None], size=(h, w), mode="bilinear", align_corners=False)[0].view(*shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--image", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rle_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    T, padded = a.frames, (a.height, a.width)
    image, output = (a.height - 8, a.width - 8), padded
    g = torch.Generator().manual_seed(0)
    cls = torch.randn(1, Q, K + 1, generator=g).to(dev)
    head = VideoMaskFormerInference(K, TOPK)
    res = {"bench": "rle", "device": torch.cuda.get_device_name(0), "Q": Q, "K": K, "reps": a.reps,
           "video": {"frames": T, "padded": list(padded), "image": list(image), "output": list(output)}}

    def video_host(out):
        r = head(out, padded, image, output, packed=True)
        r["pred_masks"] = [rle_encode(m, width=output[1]) for m in r["pred_masks"]]
        return r

    for kind in ("noise", "blobs"):
        masks = logits((1, Q, T, a.height // 4, a.width // 4), kind, g).to(dev)
        for name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            out = {"pred_logits": cls, "pred_masks": masks.to(dt)}
            device = lambda: head(out, padded, image, output, rle=True)  # noqa: E731
            host = lambda: video_host(out)  # noqa: E731
            got, want = device(), host()
            if got["pred_masks"] != want["pred_masks"] or got["pred_scores"] != want["pred_scores"]:
                raise SystemExit(f"rle_bench: the device and host routes disagree ({kind} {name} video)")
            r = both(device, host, a.reps)
            r["encoded_bytes"] = sum(len(e["counts"]) for m in got["pred_masks"] for e in m)
            res["video"][f"{kind}_{name}"] = r
        del masks

    side = a.image
    icls = torch.randn(1, Q, K + 1, generator=g).to(dev)
    ihead = MaskFormerInference(num_classes=K, semantic_on=False, instance_on=True, test_topk_per_image=100)
    iout = {"pred_logits": icls, "pred_masks": None}

    def image_device():
        return ihead(iout, (side, side), [(side, side)], instance_rle=True)[0]["instances"]["pred_masks_rle"]

    def image_host():
        return rle_encode((ihead(iout, (side, side), [(side, side)])[0]["instances"]["pred_masks"] > 0).cpu())

    res["image"] = {"size": [side, side]}
    for kind in ("noise", "blobs"):
        iout["pred_masks"] = logits((1, Q, side // 4, side // 4), kind, g).to(dev)
        got = image_device()
        if got != image_host():
            raise SystemExit(f"rle_bench: the device and host routes disagree ({kind} image)")
        res["image"][kind] = {"detections": len(got), **both(image_device, image_host, max(2, a.reps // 3)),
                              "encoded_bytes": sum(len(r["counts"]) for r in got)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
