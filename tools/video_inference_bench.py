"""Time the fused video inference head and the DINO feature resize against the reference formulation written in
torch on the same GPU, in the same run (video_maskformer_model.py:372-393 + :651-694, and :506-517).

    python tools/video_inference_bench.py [--frames 8] [--height 480] [--width 640] [--reps 10]
                                          [--out profiles/video_inference.json]

Inference: Q = 100, K = 40, one clip of --frames frames padded to --height x --width (the image is 8 pixels smaller
each way and the output is the padded size, so both resize stages run), logits at a quarter of the padded size, fp32
and fp16.  `fused` is VideoMaskFormerInference (bool and packed form), `torch` is the F.interpolate chain on the
selected queries -- the baseline gathers the ten queries first, which the reference does only after upsampling all Q
-- followed by `> 0` and `.cpu()`.  Resize: D = 128 features of the image size inside the padded size, to stride 4;
`torch` is the zero-padded copy plus F.interpolate.  Each entry is milliseconds per call between two device events
around --reps calls after warm-up (the faster of two alternated windows), including the Python glue and the one
device-to-host copy; `peak_bytes` is the rise of torch.cuda.max_memory_allocated over one call.  Needs a HIP device;
prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import VideoMaskFormerInference, feat_resize_pad  # noqa: E402

Q, K, TOPK, D = 100, 40, 10, 128


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


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


def both(fused, base, reps):
    t = [timed(fused, reps), timed(base, reps), timed(fused, reps), timed(base, reps)]
    tf, tb = min(t[0], t[2]), min(t[1], t[3])
    return {"fused_ms": round(tf, 4), "torch_ms": round(tb, 4), "speedup": round(tb / tf, 2),
            "fused_peak_bytes": peak(fused), "torch_peak_bytes": peak(base)}


def torch_video(cls, masks, padded, image, output):
    """inference_video on the ten selected queries only."""
    scores = F.softmax(cls, dim=-1)[:, :-1]
    s, idx = scores.flatten(0, 1).topk(TOPK, sorted=False)
    m = F.interpolate(masks[idx // K].float(), size=padded, mode="bilinear", align_corners=False)
    m = F.interpolate(m[:, :, :image[0], :image[1]], size=output, mode="bilinear", align_corners=False)
    return s.tolist(), (idx % K).tolist(), [x for x in (m > 0).cpu()]


def torch_resize(feats, padded, out):
    T, Dm, Hs, Ws = feats.shape
    full = torch.zeros((T, Dm, *padded), dtype=torch.float32, device=feats.device)
    full[:, :, :Hs, :Ws] = feats
    return F.interpolate(full, size=out, mode="bilinear", align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_inference_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    T, padded = a.frames, (a.height, a.width)
    image, output = (a.height - 8, a.width - 8), padded
    g = torch.Generator().manual_seed(0)
    cls = torch.randn(1, Q, K + 1, generator=g).to(dev)
    masks = (torch.randn(1, Q, T, a.height // 4, a.width // 4, generator=g) * 3).to(dev)
    head = VideoMaskFormerInference(K, TOPK)
    res = {"bench": "video_inference", "device": torch.cuda.get_device_name(0), "Q": Q, "K": K, "frames": T,
           "padded": list(padded), "image": list(image), "output": list(output), "reps": a.reps,
           "reference_upsampled_bytes": Q * T * padded[0] * padded[1] * 4, "inference": {}, "resize": {}}
    for name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
        out = {"pred_logits": cls, "pred_masks": masks.to(dt)}
        base = lambda: torch_video(cls[0], out["pred_masks"][0], padded, image, output)  # noqa: E731
        res["inference"][name] = {
            "bool": both(lambda: head(out, padded, image, output), base, a.reps),
            "packed": both(lambda: head(out, padded, image, output, packed=True), base, a.reps)}
        feats = torch.randn(T, D, *image, device=dev).to(dt)
        small = (padded[0] // 4, padded[1] // 4)
        res["resize"][name] = both(lambda: feat_resize_pad(feats, padded, small),
                                   lambda: torch_resize(feats, padded, small), a.reps)
        del feats
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
