"""Time training on label-map targets against the best route without them, on the same commit and device.

    python tools/label_targets_bench.py [--out profiles/label_targets.json] [--reps 30]

One ``SetCriterion.forward + backward`` with three heads (main plus two aux), ``num_points`` 12544, oversample ratio
3.0, importance ratio 0.75, from panoptic / semantic maps that already lie on the device:

(a) label   ``panoptic_targets`` / ``semantic_targets`` (timed with the step and also on their own), then the
            criterion on the label-map targets;
(b) dense   the masks built on the device with one broadcast ``==`` per image into a zero-padded (G, h_pad, w_pad)
            uint8 tensor, as ``prepare_targets`` pads them, then the criterion's existing dense path.  The ids and
            classes route (b) compares against are known to it beforehand and cost it nothing.

Workloads: COCO-panoptic-like, 16 maps of 1024 x 1024 (int32 ids, about 20 segments each), Q = 100, masks 256 x 256;
ADE20K-like, 16 maps of 512 x 512 (uint8 classes, about 10 of 150 each), Q = 100, masks 128 x 128.

Timed: host clock around the whole step between two device synchronisations, after two warm-up steps; the faster of
two windows of ``reps`` steps each is reported as ms per step.  Not timed: building the maps, reading files, the
model.  Peak memory is ``torch.cuda.max_memory_allocated`` over one step above what is allocated before it (the maps
and predictions).  Launches are counted with torch.profiler in a step of their own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import HungarianMatcher, SetCriterion, panoptic_targets, semantic_targets  # noqa: E402

HEADS, K, RATIO, IMPORTANCE = 3, 12544, 3.0, 0.75
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
WORKLOADS = {
    "coco_panoptic_like": {"kind": "panoptic", "B": 16, "size": 1024, "segments": 20, "classes": 133, "Q": 100,
                           "mask": 256, "dtype": "int32"},
    "ade20k_like": {"kind": "semantic", "B": 16, "size": 512, "segments": 10, "classes": 150, "Q": 100, "mask": 128,
                    "dtype": "uint8"},
}
IGNORE = 255


def make_maps(w, dev):
    """Voronoi-like maps: every pixel takes the id of the nearest of `segments` random seeds; a band is VOID / ignored."""
    g = torch.Generator().manual_seed(0)
    n, S = w["size"], w["segments"]
    yy, xx = torch.meshgrid(torch.arange(n).float(), torch.arange(n).float(), indexing="ij")
    maps, infos = [], []
    for _ in range(w["B"]):
        seeds = torch.rand(S, 2, generator=g) * n
        near = ((yy[None] - seeds[:, 0, None, None]) ** 2 + (xx[None] - seeds[:, 1, None, None]) ** 2).argmin(0)
        if w["kind"] == "panoptic":
            ids = torch.randint(1, 2 ** 24, (S,), generator=g)
            cats = torch.randint(0, w["classes"], (S,), generator=g)
            m = ids[near]
            m[:, : n // 32] = 0                                                   # VOID
            infos.append([{"id": int(i), "category_id": int(c), "iscrowd": 0} for i, c in zip(ids, cats)])
        else:
            m = torch.randperm(w["classes"], generator=g)[:S][near]
            m[:, : n // 32] = IGNORE
        maps.append(m.to(getattr(torch, w["dtype"])).to(dev))
    return maps, infos


def weighted(losses):
    return sum(v.sum() * WEIGHTS[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k, v in losses.items())


def windows(fn, reps):
    for _ in range(2):
        fn()
    best = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"ms_per_step": min(best), "windows_ms": best, "steps_per_window": reps}


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def bench(w, dev, reps):
    maps, infos = make_maps(w, dev)
    g = torch.Generator().manual_seed(1)
    heads = [{"pred_logits": torch.randn(w["B"], w["Q"], w["classes"] + 1, generator=g).to(dev),
              "pred_masks": (torch.randn(w["B"], w["Q"], w["mask"], w["mask"], generator=g) * 3).to(dev)}
             for _ in range(HEADS)]
    matcher = HungarianMatcher(2.0, 5.0, 5.0, K)
    crit = SetCriterion(w["classes"], matcher, WEIGHTS, 0.1, ["labels", "masks"], K, RATIO, IMPORTANCE).to(dev)

    def helper():
        if w["kind"] == "panoptic":
            return panoptic_targets(maps, infos)
        return semantic_targets(maps, IGNORE, w["classes"])

    known = [{"labels": t["labels"], "ids": t["ids"]} for t in helper()]            # route (b) is given these
    pad = max(m.shape[0] for m in maps), max(m.shape[1] for m in maps)

    def dense_targets():
        out = []
        for m, t in zip(maps, known):
            masks = torch.zeros((t["ids"].shape[0], *pad), dtype=torch.uint8, device=dev)
            masks[:, : m.shape[0], : m.shape[1]] = m[None] == t["ids"][:, None, None]
            out.append({"labels": t["labels"], "masks": masks})
        return out

    def step(make):
        hs = [{k: v.detach().requires_grad_() for k, v in h.items()} for h in heads]
        weighted(crit(dict(hs[-1], aux_outputs=hs[:-1]), make())).backward()

    res = {"shapes": dict(w, heads=HEADS, num_points=K, oversample_ratio=RATIO, importance_sample_ratio=IMPORTANCE,
                          targets_per_image=[int(t["ids"].shape[0]) for t in known])}
    held = {"label": sum(m.numel() * m.element_size() for m in maps) + sum(4 * t["ids"].numel() for t in known),
            "dense": sum(t["ids"].shape[0] * pad[0] * pad[1] for t in known)}
    for name, make in (("label", helper), ("dense", dense_targets)):
        res[name] = {"step": windows(lambda: step(make), reps), "targets_only": windows(make, reps),
                     "peak_bytes_above_inputs": peak_of(lambda: step(make)), "launches_per_step": launches_of(lambda: step(make)),
                     "target_bytes_held": held[name]}
    res["dense_over_label_step_time"] = res["dense"]["step"]["ms_per_step"] / res["label"]["step"]["ms_per_step"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_targets.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_targets_bench needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "timed": "host clock around forward + backward of a 3-head SetCriterion, target construction included, "
                    "between device synchronisations; faster of two windows after two warm-up steps",
           "not_timed": "building the maps, file reading, the model"}
    for name, w in WORKLOADS.items():
        res[name] = bench(w, dev, a.reps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {r: {"ms_per_step": res[n][r]["step"]["ms_per_step"],
                              "targets_only_ms": res[n][r]["targets_only"]["ms_per_step"],
                              "peak_bytes": res[n][r]["peak_bytes_above_inputs"],
                              "launches": res[n][r]["launches_per_step"]} for r in ("label", "dense")}
                      for n in WORKLOADS}))


if __name__ == "__main__":
    main()
