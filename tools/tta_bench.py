"""Time the fused semantic test-time-augmentation head (csrc/semantic_tta.hip under ``semantic_inference_tta``) against
the best route without it and against the reference-style route.

    python tools/tta_bench.py [--reps 10] [--ref-reps 3] [--out profiles/semantic_tta.json]

Shapes (synthetic, seeded; the low-resolution logits of every view start on the device, as the model leaves them; a
view is padded to a multiple of 32 and its logits are a quarter of the padded size):

    ade20k      K = 150, Q = 100, image 512 x 683, TEST.AUG of the ADE20K semantic configs: MIN_SIZES 256 .. 896,
                MAX_SIZE 3584, FLIP -> V = 12
    cityscapes  K = 19, Q = 100, image 1024 x 2048, MIN_SIZES 512 .. 1792, MAX_SIZE 4096, FLIP -> V = 12

Routes, each in both orders (``before`` = sem_seg_postprocess_before_inference, ``after`` = the configs' default) and
for scores and for labels:

    fused       one call of semantic_inference_tta
    per_view    V calls of the existing fused semantic head (m2f_infer_semantic; in the `after` order on the crop,
                then F.interpolate of its (K, Hc, Wc) scores), ``flip``, ``add_`` into a running sum, ``div``;
                ``argmax`` for labels.  The best route this repository had before the fused head.
    reference   the reference's arithmetic in torch: F.interpolate of the (Q, h, w) logits to the padded size, crop,
                sigmoid, einsum with the class probabilities, resize (before or after), flip, add, div

Per route: ``ms`` wall milliseconds per call (host clock, a device synchronise before and after), the faster of two
windows of --reps calls (--ref-reps for the reference route) after one warm-up call, ``windows_ms`` both windows (their
gap is the run-to-run spread a comparison has to exceed), and ``peak_mb`` torch.cuda.max_memory_allocated over one
call minus the level before it.  The fused route is checked against per_view first (1e-3 of the maximum).

What this does not measure: kernel time.  No device events and no profiler trace are taken; ``ms`` includes the
host's launch work (for per_view about 5 V small launches).  The inputs are re-used every call: the ADE20K logits
(148 MB) and its 210 MB score tensor each fit the 256 MB Infinity Cache, so re-reads of either route may be served
from it there; the cityscapes logits (911 MB) and its per-view score tensors in the `after` order (up to 488 MB) do
not.  Needs a HIP device; prints one JSON line."""
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
from bm2f_amd import semantic_inference_tta, tta_view_sizes  # noqa: E402
from bm2f_amd.inference import _semantic_hip  # noqa: E402

SHAPES = {
    "ade20k": dict(K=150, Q=100, image=(512, 683), min_sizes=(256, 384, 512, 640, 768, 896), max_size=3584),
    "cityscapes": dict(K=19, Q=100, image=(1024, 2048), min_sizes=(512, 768, 1024, 1280, 1536, 1792), max_size=4096),
}


def windows(fn, reps):
    out = []
    fn()
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return out


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak / 2 ** 20


def make_views(s, dev, g):
    views = []
    for h, w, flipped in tta_view_sizes(*s["image"], s["min_sizes"], s["max_size"], True):
        hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
        cls = torch.randn(s["Q"], s["K"] + 1, generator=g).to(dev)
        masks = (torch.randn(s["Q"], hp // 4, wp // 4, generator=g) * 3).to(dev)
        views.append(({"pred_logits": cls, "pred_masks": masks}, (hp, wp), (h, w), flipped))
    return views


def per_view(views, out, before, labels):
    total = None
    for o, padded, (hc, wc), flipped in views:
        geo = [(hc, wc, *out)] if before else [(hc, wc, hc, wc)]
        r = _semantic_hip(o["pred_logits"][None], o["pred_masks"][None], padded, geo)[0]
        if not before and (hc, wc) != out:
            r = F.interpolate(r[None], size=out, mode="bilinear", align_corners=False)[0]
        if flipped:
            r = r.flip(-1)
        total = r if total is None else total.add_(r)
    total = total.div_(len(views))
    return total.argmax(0).to(torch.int16) if labels else total


def reference_style(views, out, before, labels):
    total = None
    for o, padded, (hc, wc), flipped in views:
        probs = F.softmax(o["pred_logits"], dim=-1)[..., :-1]
        m = F.interpolate(o["pred_masks"][None], size=padded, mode="bilinear", align_corners=False)[0]
        if before:
            m = F.interpolate(m[None, :, :hc, :wc], size=out, mode="bilinear", align_corners=False)[0]
            r = torch.einsum("qc,qhw->chw", probs, m.sigmoid())
        else:
            r = torch.einsum("qc,qhw->chw", probs, m.sigmoid())
            r = F.interpolate(r[None, :, :hc, :wc], size=out, mode="bilinear", align_corners=False)[0]
        del m
        if flipped:
            r = r.flip(dims=[2])
        total = r if total is None else total + r
    total = total / len(views)
    return total.argmax(0).to(torch.int16) if labels else total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="calls per window of the fused and per_view routes")
    ap.add_argument("--ref-reps", type=int, default=3, help="calls per window of the reference-style route")
    ap.add_argument("--shapes", default="ade20k,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"bench": "semantic_tta", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ref_reps": a.ref_reps,
           "kernel_time_taken": False}
    for name in a.shapes.split(","):
        s = SHAPES[name]
        views = make_views(s, dev, g)
        out = s["image"]
        entry = {"K": s["K"], "Q": s["Q"], "output": list(out), "views": [[*v[2], int(v[3])] for v in views],
                 "score_tensor_mb": round(s["K"] * out[0] * out[1] * 4 / 2 ** 20, 1)}
        for order, before in (("before", True), ("after", False)):
            fused = semantic_inference_tta(views, out, num_classes=s["K"], before=before)
            base = per_view(views, out, before, False)
            err = ((fused - base).abs().max() / base.abs().max()).item()
            assert err < 1e-3, (name, order, err)
            del fused, base
            for what, labels in (("scores", False), ("labels", True)):
                routes = {"fused": (lambda: semantic_inference_tta(views, out, num_classes=s["K"], before=before,
                                                                    labels=labels), a.reps),
                          "per_view": (lambda: per_view(views, out, before, labels), a.reps),
                          "reference": (lambda: reference_style(views, out, before, labels), a.ref_reps)}
                row = {}
                for route, (fn, reps) in routes.items():
                    w = windows(fn, reps)
                    row[route] = {"ms": round(min(w), 3), "windows_ms": [round(x, 3) for x in w],
                                  "peak_mb": round(peak_mb(fn), 1)}
                row["per_view_over_fused"] = round(row["per_view"]["ms"] / row["fused"]["ms"], 2)
                row["reference_over_fused"] = round(row["reference"]["ms"] / row["fused"]["ms"], 2)
                entry[f"{order}_{what}"] = row
            entry[f"{order}_fused_vs_per_view_rel_err"] = err
        res[name] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
