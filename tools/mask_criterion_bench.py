"""Time the mask-supervised matcher and criterion against a torch restatement of the reference on the same device.

    python tools/mask_criterion_bench.py [--out profiles/mask_criterion.json] [--reps 5]

Two shape sets, per rank:

* image (benchmark config 2): B = 16, Q = 100, masks 256 x 256, uint8 targets 1024 x 1024 (12 per image),
  num_points 12544, oversample ratio 3, importance ratio 0.75, 10 decoder heads;
* video (benchmark config 5 clips): B = 2, Q = 100, T = 5, masks 96 x 160, uint8 targets 384 x 640 (8 per clip),
  the same point settings, 10 heads.

Two parts are timed for each, as the median of ``reps`` runs after two warm-up runs with a device synchronisation
around every run: one head's matching, and the criterion's forward + backward over all heads (matching included).
The restatement follows the reference's structure: a per-image loop that converts the targets to float, samples
with ``F.grid_sample`` on (N, 1, H, W) gathers, copies each cost matrix to the host and calls scipy; the losses
gather ``pred_masks[src_idx]``, pad and convert the full-resolution targets once per head.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd.mask_criterion import (HungarianMatcher, SetCriterion, VideoHungarianMatcher,  # noqa: E402
                                     VideoSetCriterion, point_sample)

CLASSES, HEADS, K, RATIO, IMPORTANCE = 80, 10, 12544, 3.0, 0.75
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
SHAPES = {"image": {"B": 16, "Q": 100, "T": 0, "H": 256, "W": 256, "Ht": 1024, "Wt": 1024, "G": 12},
          "video": {"B": 2, "Q": 100, "T": 5, "H": 96, "W": 160, "Ht": 384, "Wt": 640, "G": 8}}


def timed(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def make_inputs(s, dev):
    g = torch.Generator().manual_seed(0)
    B, Q, T, H, W, Ht, Wt, G = (s[k] for k in ("B", "Q", "T", "H", "W", "Ht", "Wt", "G"))
    targets = []
    yy, xx = torch.meshgrid(torch.arange(Ht).float(), torch.arange(Wt).float(), indexing="ij")
    for _ in range(B):
        m = torch.zeros((G, max(T, 1), Ht, Wt), dtype=torch.uint8)
        for i in range(G):
            cy, cx, ry, rx = (float(v) for v in torch.rand(4, generator=g))
            for t in range(max(T, 1)):
                m[i, t] = (((yy - cy * Ht - 2 * t) / ((0.05 + 0.25 * ry) * Ht)) ** 2
                           + ((xx - cx * Wt + 3 * t) / ((0.05 + 0.25 * rx) * Wt)) ** 2 <= 1.0)
        targets.append({"labels": torch.randint(0, CLASSES, (G,), generator=g).to(dev),
                        "masks": (m if T else m[:, 0]).to(dev)})
    lead = (B, Q, T) if T else (B, Q)
    heads = [{"pred_logits": torch.randn(B, Q, CLASSES + 1, generator=g).to(dev),
              "pred_masks": (torch.randn(*lead, H, W, generator=g) * 3).to(dev)} for _ in range(HEADS)]
    return targets, heads


# -- the reference, restated ---------------------------------------------------------------------------------
def ref_match(head, targets, video):
    from scipy.optimize import linear_sum_assignment
    out = []
    for b, t in enumerate(targets):
        prob = head["pred_logits"][b].softmax(-1)
        c_class = -prob[:, t["labels"]]
        x = head["pred_masks"][b]
        m = t["masks"].to(x)
        if not video:
            x, m = x[:, None], m[:, None]
        u = torch.rand(1, K, 2, device=x.device)
        m = point_sample(m, u.repeat(m.shape[0], 1, 1)).flatten(1)
        x = point_sample(x, u.repeat(x.shape[0], 1, 1)).flatten(1)
        pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
        neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
        c_mask = (pos @ m.t() + neg @ (1 - m).t()) / x.shape[1]
        s = x.sigmoid()
        c_dice = 1 - (2 * s @ m.t() + 1) / (s.sum(-1)[:, None] + m.sum(-1)[None] + 1)
        C = 5.0 * c_mask + 2.0 * c_class + 5.0 * c_dice
        i, j = linear_sum_assignment(C.cpu())
        out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
    return out


def ref_losses(head, targets, idx, num_masks, video):
    dev = head["pred_masks"].device
    B, Q = head["pred_logits"].shape[:2]
    bi = torch.cat([torch.full_like(s, b) for b, (s, _) in enumerate(idx)])
    si = torch.cat([s for s, _ in idx])
    cls = torch.full((B, Q), CLASSES, dtype=torch.int64, device=dev)
    cls[bi, si] = torch.cat([t["labels"][j] for t, (_, j) in zip(targets, idx)])
    wt = torch.ones(CLASSES + 1, device=dev)
    wt[-1] = 0.1
    out = {"loss_ce": F.cross_entropy(head["pred_logits"].transpose(1, 2), cls, wt)}
    src = head["pred_masks"][bi, si]
    if video:
        tgt = torch.cat([t["masks"][j] for t, (_, j) in zip(targets, idx)]).to(src)
        src, tgt = src.flatten(0, 1)[:, None], tgt.flatten(0, 1)[:, None]
    else:
        tj = torch.cat([j for _, j in idx])
        tgt = torch.stack([t["masks"] for t in targets]).to(src)[bi, tj]      # nested tensor: same sizes here
        src, tgt = src[:, None], tgt[:, None]
    with torch.no_grad():
        n = src.shape[0]
        over = torch.rand(n, int(K * RATIO), 2, device=dev)
        unc = -point_sample(src, over)[:, 0].abs()
        n_unc = int(IMPORTANCE * K)
        top = torch.topk(unc, k=n_unc, dim=1)[1]
        top = top + int(K * RATIO) * torch.arange(n, device=dev)[:, None]
        u = over.view(-1, 2)[top.view(-1)].view(n, n_unc, 2)
        u = torch.cat([u, torch.rand(n, K - n_unc, 2, device=dev)], 1)
        lab = point_sample(tgt, u)[:, 0]
    x = point_sample(src, u)[:, 0]
    out["loss_mask"] = F.binary_cross_entropy_with_logits(x, lab, reduction="none").mean(1).sum() / num_masks
    s = x.sigmoid()
    out["loss_dice"] = (1 - (2 * (s * lab).sum(-1) + 1) / (s.sum(-1) + lab.sum(-1) + 1)).sum() / num_masks
    return out


def weighted(losses):
    return sum(v.sum() * WEIGHTS[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k, v in losses.items())


def bench(name, s, dev, reps):
    video = bool(s["T"])
    targets, heads = make_inputs(s, dev)
    matcher = (VideoHungarianMatcher if video else HungarianMatcher)(2.0, 5.0, 5.0, K).to(dev)
    args = (CLASSES, matcher, WEIGHTS, 0.1, ["labels", "masks"], K, RATIO, IMPORTANCE)
    crit = (VideoSetCriterion(*args) if video else SetCriterion(*args, "mask")).to(dev)
    res = {"shapes": dict(s, classes=CLASSES, heads=HEADS, num_points=K, oversample_ratio=RATIO,
                          importance_sample_ratio=IMPORTANCE)}
    res["matcher_one_head"] = {"hip": timed(lambda: matcher(heads[0], targets), reps),
                               "torch_reference": timed(lambda: ref_match(heads[0], targets, video), reps)}

    def ours():
        hs = [{k: v.detach().requires_grad_() for k, v in h.items()} for h in heads]
        weighted(crit(dict(hs[-1], aux_outputs=hs[:-1]), targets)).backward()

    def theirs():
        hs = [{k: v.detach().requires_grad_() for k, v in h.items()} for h in heads]
        num_masks = float(s["B"] * s["G"])
        total = 0
        for h in [hs[-1]] + hs[:-1]:
            with torch.no_grad():
                idx = [(i.to(dev), j.to(dev)) for i, j in ref_match(h, targets, video)]
            total = total + weighted(ref_losses(h, targets, idx, num_masks, video))
        total.backward()

    res["criterion_fwd_bwd_10_heads"] = {"hip": timed(ours, reps), "torch_reference": timed(theirs, reps)}
    for k in ("matcher_one_head", "criterion_fwd_bwd_10_heads"):
        res[k]["torch_over_hip"] = res[k]["torch_reference"]["median_ms"] / res[k]["hip"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_criterion.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_criterion_bench needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    for name, s in SHAPES.items():
        res[name] = bench(name, s, dev, a.reps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {k: res[n][k]["torch_over_hip"] for k in ("matcher_one_head", "criterion_fwd_bwd_10_heads")}
                      for n in SHAPES}))


if __name__ == "__main__":
    main()
