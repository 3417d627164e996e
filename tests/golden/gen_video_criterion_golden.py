"""Generate tests/golden/video_criterion.npz by running the REFERENCE box-supervised video criterion on the
CPU (nothing from the reference tree is copied).

    python tests/golden/gen_video_criterion_golden.py --ref /path/to/reference

Imported in place with the stand-ins of gen_criterion_golden.install_weaksup_stubs:
  * VideoHungarianMatcherProjPair (mask2former_video/modeling/matcher.py:249-393) and
    VideoSetCriterionProjSpatPairTempPair (modeling/criterion_proj_spatpair_temppair.py:72-406) with 3 decoder
    heads (2 aux), pairwise warm-up over 3 iterations, run for 4 -> matched indices per head, every loss, and
    the gradients of the weighted loss sum w.r.t. pred_logits / pred_masks;
  * get_instance_temporal_pairs (utils/weaksup_utils.py:157-165) looped over instances and frame pairs as
    video_maskformer_model.py:523-558 does -> the mined pairs (also the criterion's ``temporal_pairs``).

Shapes: B = 2 clips, T = 3, Q = 6, 5 classes, masks 24 x 40, D = 16.  Clip 0 has 3 targets, one of them absent
from the middle frame (all-zero box, no pairs across that frame); clip 1 has 1 target.  Mask logits are
multiples of 1/16 below 13 in magnitude plus +-40 patches, so they are exact in fp16 and the file stores them as
int16 (similarities and features are stored as uint8 / 255 and int8 / 16 likewise, to keep the file small); the
generator keeps every row / column maximum of every mask unique, so the projection gradient's arg-max has no ties
to break.

Asserted here, for the reference alone: every stored assignment is unchanged under a 1e-5 relative perturbation of
its cost matrix; at most 10 % of the mined rows are ambiguous, i.e. have more than one next-box pixel whose fp64
distance d satisfies d <= d_min (1 + 2^-9) + cdist_abs_err (2^-9: one fp16 ulp, from the reference's .half()
before topk; cdist_abs_err: the measured error of the reference's fp32 cdist against fp64 on these inputs).
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from gen_criterion_golden import install_weaksup_stubs  # noqa: E402

B, T, Q, K, H, W, D = 2, 3, 6, 5, 24, 40, 16
N_AUX, ITERS, WARMUP = 2, 4, 3
WEIGHTS = {"loss_ce": 2.0, "loss_mask_projection": 5.0, "loss_mask_spatial_pairwise": 5.0,
           "loss_mask_temporal_pairwise": 3.0}
LOSS_ORDER = ("loss_ce", "loss_mask_projection", "loss_mask_spatial_pairwise", "loss_mask_temporal_pairwise")
MASK_SCALE = 16          # masks are stored as int16 = logit * 16
FEAT_SCALE = 16          # features as int8 = feature * 16
SIM_SCALE = 255          # colour similarities as uint8 = similarity * 255
# integer XYXY boxes per clip, target and frame, half-open; up to 12 x 9, one 1 x 1, one touching the frame edge
BOXES = [
    [[[2, 3, 14, 12], [4, 4, 15, 12], [5, 5, 16, 13]],
     [[20, 2, 29, 9], [0, 0, 0, 0], [22, 4, 30, 11]],            # absent from the middle frame
     [[30, 15, 40, 24], [31, 16, 40, 24], [33, 17, 34, 18]]],    # frame edge; 1 x 1 in the last frame
    [[[8, 6, 19, 15], [9, 7, 20, 15], [10, 8, 21, 16]]],
]
LABELS = [[1, 4, 0], [2]]


def import_reference(ref_root):
    install_weaksup_stubs()
    sys.path.insert(0, ref_root)
    for pkg in ("mask2former", "mask2former.modeling", "mask2former.utils", "mask2former_video",
                "mask2former_video.modeling", "mask2former_video.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
        sys.modules[pkg] = m
    return types.SimpleNamespace(
        matcher=importlib.import_module("mask2former_video.modeling.matcher"),
        criterion=importlib.import_module("mask2former_video.modeling.criterion_proj_spatpair_temppair"),
        wsu=importlib.import_module("mask2former_video.utils.weaksup_utils"))


def unique_maxima(k):
    """Bump entries of the integer masks k (..., H, W) until every row and column maximum is unique."""
    for _ in range(200):
        changed = False
        for dim in (-1, -2):
            m = k.amax(dim, keepdim=True)
            tie = (k == m)
            multi = tie.sum(dim, keepdim=True) > 1
            first = tie & (tie.cumsum(dim) == 1) & multi
            if first.any():
                k = k + first.to(k.dtype)
                changed = True
        if not changed:
            return k
    raise AssertionError("could not make the axis maxima unique")


def make_masks(gen, boxes_b):
    """int16 mask logits (B, Q, T, H, W) * MASK_SCALE: noise, box-like blobs on some queries, +-40 patches."""
    k = (torch.randn(B, Q, T, H, W, generator=gen) * 3 * MASK_SCALE).round().clamp(-12 * MASK_SCALE, 12 * MASK_SCALE)
    for b in range(B):
        for g, per_t in enumerate(boxes_b[b]):
            q = int(torch.randint(0, Q, (1,), generator=gen))
            for t, (x0, y0, x1, y1) in enumerate(per_t):
                k[b, q, t, y0:y1, x0:x1] += 4 * MASK_SCALE
    k = unique_maxima(k.to(torch.int64))
    # saturated patches after the uniqueness pass (sigmoid(40) == 1 in fp32: their gradient is exactly 0)
    k[:, 0, :, :3, :3] = 40 * MASK_SCALE
    k[:, 1, :, -2:, :] = -40 * MASK_SCALE
    k[:, 2, 1, 10:12, 20:23] = 40 * MASK_SCALE
    assert int(k.abs().max()) <= 40 * MASK_SCALE
    return k.to(torch.int16)


def mine(ref, feats, boxes):
    """video_maskformer_model.py:523-558 for one clip: feats (T, D, H, W), boxes (G, T, 4) int64."""
    out, err = [], 0.0
    for g in range(boxes.shape[0]):
        bx = boxes[g]
        pos = ((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])) > 0
        per = []
        for i in range(T - 1):
            if pos[i:i + 2].all():
                cur, nxt = ref.wsu.get_instance_temporal_pairs(feats[i:i + 2], bx[i:i + 2], k=1)
                a, b = ref.wsu.get_obj_feats(feats[i:i + 2], bx[i:i + 2])
                a, b = a.flatten(1).t(), b.flatten(1).t()
                d64 = torch.cdist(a.double(), b.double(), p=2)
                err = max(err, float((torch.cdist(a, b, p=2).double() - d64).abs().max()))
                per.append((cur, nxt, d64))
            else:
                per.append((torch.zeros((0, 2), dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32), None))
        out.append(per)
    return out, err


def gen_all(ref, out_dir):
    gen = torch.Generator().manual_seed(2024)
    res = {"B": B, "T": T, "Q": Q, "K": K, "H": H, "W": W, "D": D, "n_aux": N_AUX, "iters": ITERS, "warmup": WARMUP,
           "mask_scale": MASK_SCALE, "feat_scale": FEAT_SCALE, "sim_scale": SIM_SCALE,
           "weights": np.array([WEIGHTS[k] for k in LOSS_ORDER])}
    targets, cdist_err, mined = [], 0.0, []
    for b in range(B):
        boxes = torch.tensor(BOXES[b], dtype=torch.int64)                                  # (G, T, 4)
        G = boxes.shape[0]
        bm = torch.zeros(G, T, H, W)
        for g in range(G):
            for t in range(T):
                x0, y0, x1, y1 = boxes[g, t].tolist()
                bm[g, t, y0:y1, x0:x1] = 1.0
        sim_q = torch.randint(0, 256, (T, 8, H, W), generator=gen).to(torch.uint8)
        sim = sim_q.float() / SIM_SCALE
        # smooth field + noise: neighbouring pixels are similar but distinct
        base = torch.randn(T, D, H // 4 + 1, W // 4 + 1, generator=gen).repeat_interleave(4, 2) \
            .repeat_interleave(4, 3)[:, :, :H, :W]
        feats_q = ((base + torch.randn(T, D, H, W, generator=gen)) * FEAT_SCALE).round().clamp(-127, 127)
        feats_q = feats_q.to(torch.int8)
        feats = feats_q.float() / FEAT_SCALE
        pairs, err = mine(ref, feats, boxes)
        cdist_err = max(cdist_err, err)
        mined.append(pairs)
        targets.append({"labels": torch.tensor(LABELS[b]), "box_masks": bm,
                        "color_similarities": sim[None].repeat(G, 1, 1, 1, 1),
                        "temporal_pairs": [[(c, n) for c, n, _ in per] for per in pairs]})
        res[f"boxes{b}"] = boxes.numpy()
        res[f"labels{b}"] = np.array(LABELS[b], np.int64)
        res[f"box_masks{b}"] = bm.numpy().astype(np.uint8)
        res[f"sim{b}"] = sim_q.numpy()
        res[f"feats{b}"] = feats_q.numpy()
        packed = [(g, t, c[:, 0], c[:, 1], n[:, 0], n[:, 1]) for g, per in enumerate(pairs)
                  for t, (c, n, _) in enumerate(per) if c.shape[0]]
        res[f"pairs{b}"] = np.concatenate(
            [np.stack([np.full(len(cx), g), np.full(len(cx), t), cx, cy, nx, ny], 1) for g, t, cx, cy, nx, ny in packed]
        ).astype(np.int32)                                                                  # (P, 6) g t cx cy nx ny
    res["cdist_abs_err"] = np.float64(cdist_err)
    # ambiguity of the mined rows under the tests' admissibility rule
    rows = ambiguous = 0
    for b in range(B):
        for per in mined[b]:
            for c, n, d64 in per:
                if d64 is None:
                    continue
                ok = d64 <= d64.amin(1, keepdim=True) * (1 + 2.0 ** -9) + cdist_err
                rows += d64.shape[0]
                ambiguous += int((ok.sum(1) > 1).sum())
    print(f"mined rows {rows}, ambiguous {ambiguous}, cdist_abs_err {cdist_err:.3e}")
    assert ambiguous <= 0.10 * rows, "too many ambiguous mined rows: scale the features or change the seed"

    matcher = ref.matcher.VideoHungarianMatcherProjPair(
        cost_class=WEIGHTS["loss_ce"], cost_projection=WEIGHTS["loss_mask_projection"],
        cost_pairwise=WEIGHTS["loss_mask_spatial_pairwise"], pairwise_size=3, pairwise_dilation=2,
        pairwise_color_thresh=0.3, pairwise_warmup_iters=WARMUP)
    crit = ref.criterion.VideoSetCriterionProjSpatPairTempPair(
        K, matcher=matcher, weight_dict=WEIGHTS, eos_coef=0.1, pairwise_size=3, pairwise_dilation=2,
        pairwise_color_thresh=0.3, pairwise_warmup_iters=WARMUP,
        losses=["labels", "projection_masks", "spatial_pairwise", "temporal_pairwise"])
    res["state_keys"] = np.array(sorted(crit.state_dict().keys()))
    calls = []
    lsa = ref.matcher.linear_sum_assignment
    pert = np.random.default_rng(5)

    def spy(C):
        r = lsa(C)
        c = np.asarray(C, dtype=np.float64)
        for _ in range(16):
            p = c * (1 + 1e-5 * pert.choice([-1.0, 1.0], c.shape))
            assert all(np.array_equal(x, y) for x, y in zip(lsa(p), r)), "assignment is not stable: change the seed"
        calls.append(r)
        return r

    ref.matcher.linear_sum_assignment = spy
    for it in range(ITERS):
        heads = []
        for hd in range(N_AUX + 1):
            lg = (torch.randn(B, Q, K + 1, generator=gen) * 2).requires_grad_()
            mq = make_masks(gen, BOXES)
            mk = (mq.float() / MASK_SCALE).requires_grad_()
            heads.append({"pred_logits": lg, "pred_masks": mk, "q": mq})
        outputs = {k: v for k, v in heads[-1].items() if k != "q"}
        outputs["aux_outputs"] = [{k: v for k, v in h.items() if k != "q"} for h in heads[:-1]]
        calls.clear()
        losses = crit(outputs, targets)
        total = sum(losses[k] * WEIGHTS[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k in losses)
        total.sum().backward()
        for hd, h in enumerate(heads):
            res[f"it{it}_logits{hd}"] = h["pred_logits"].detach().numpy()
            res[f"it{it}_masks{hd}"] = h["q"].numpy()
            res[f"it{it}_glogits{hd}"] = h["pred_logits"].grad.numpy()
            res[f"it{it}_gmasks{hd}"] = h["pred_masks"].grad.numpy()
        # matcher call order: final head first, then aux 0..n-1; B scipy calls per head
        order = [N_AUX] + list(range(N_AUX))
        assert len(calls) == B * len(order)
        for c, hd in enumerate(order):
            for b in range(B):
                i, j = calls[c * B + b]
                res[f"it{it}_idx{hd}_{b}"] = np.stack([i, j]).astype(np.int64)
        for k, v in losses.items():
            res[f"it{it}_{k}"] = np.float64(v.sum().item())
    res["loss_keys"] = np.array(sorted(losses.keys()))
    path = os.path.join(out_dir, "video_criterion.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < (1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    gen_all(import_reference(a.ref), a.out)


if __name__ == "__main__":
    main()
