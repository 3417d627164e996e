"""Generate tests/golden/mask_criterion.npz by running the REFERENCE mask-supervised matchers and criteria on the
CPU (nothing from the reference tree is copied).

    python tests/golden/gen_mask_criterion_golden.py --ref /path/to/reference

Imported in place with the stand-ins of gen_criterion_golden.install_weaksup_stubs plus, installed before the
reference modules are imported, stand-ins for detectron2's ``point_sample`` and
``get_uncertain_point_coords_with_randomness`` (restated from their definition: grid_sample(2u - 1, bilinear,
zeros, align_corners=False); oversample -> uncertainty -> top-k -> fresh uniform points):
  * HungarianMatcher (mask2former/modeling/matcher.py:479-597) + SetCriterion (modeling/criterion.py:775-955);
  * VideoHungarianMatcher (mask2former_video/modeling/matcher.py:503-590) + VideoSetCriterion
    (mask2former_video/modeling/criterion.py:144-310);
each with 3 decoder heads (2 aux).  ``torch.rand`` is wrapped to record every draw by kind and head.  The
reference's video matcher does not run as checked in (an undefined cost function, and a dice cost without the
sigmoid): it is run with the image matcher's two cost functions, see ``import_reference``.

Image case: B = 3, Q = 12, 5 classes, masks 20 x 28 (logits multiples of 1/16, stored as int16), targets 80 x 112
except image 1 at 64 x 96 (pins the criterion's padded-size normalisation), G = 4, 1, 2; num_points 50,
oversample ratio 3, importance ratio 0.75.  Video case: B = 2 clips, T = 3, Q = 6, masks 12 x 20, targets 48 x 80,
G = 2, 1.  Stored: the drawn coordinates, the kept top-k indices, the matched indices per head, every loss and the
gradients of the weighted loss sum w.r.t. pred_logits / pred_masks.

Asserted here, for the reference alone (seeds are retried until both hold): every assignment is unchanged under a
1e-5 relative perturbation of its cost matrix; in every row and head the gap between the last kept and the first
dropped |x| of the oversampled points is >= 1e-3, so the kept set can be compared exactly.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from gen_criterion_golden import install_weaksup_stubs  # noqa: E402

N_AUX, CLASSES = 2, 5
NUM_POINTS, OVERSAMPLE, IMPORTANCE = 50, 3.0, 0.75
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
LOSS_ORDER = ("loss_ce", "loss_mask", "loss_dice")
MASK_SCALE = 16
TOPK_GAP = 1e-3
IMAGE = {"B": 3, "Q": 12, "T": 0, "H": 20, "W": 28, "G": [4, 1, 2], "sizes": [(80, 112), (64, 96), (80, 112)]}
VIDEO = {"B": 2, "Q": 6, "T": 3, "H": 12, "W": 20, "G": [2, 1], "sizes": [(48, 80), (48, 80)]}


class Retry(Exception):
    pass


_kept = []   # per get_uncertain call: the kept indices (N, n_uncertain)


def point_sample(input, point_coords, **kwargs):
    add_dim = False
    if point_coords.dim() == 3:
        add_dim = True
        point_coords = point_coords.unsqueeze(2)
    output = F.grid_sample(input, 2.0 * point_coords - 1.0, **kwargs)
    if add_dim:
        output = output.squeeze(3)
    return output


def get_uncertain_point_coords_with_randomness(coarse_logits, uncertainty_func, num_points, oversample_ratio,
                                               importance_sample_ratio):
    assert oversample_ratio >= 1
    assert 0 <= importance_sample_ratio <= 1
    num_boxes = coarse_logits.shape[0]
    num_sampled = int(num_points * oversample_ratio)
    point_coords = torch.rand(num_boxes, num_sampled, 2, device=coarse_logits.device)
    point_logits = point_sample(coarse_logits, point_coords, align_corners=False)
    point_uncertainties = uncertainty_func(point_logits)
    num_uncertain_points = int(importance_sample_ratio * num_points)
    num_random_points = num_points - num_uncertain_points
    idx = torch.topk(point_uncertainties[:, 0, :], k=num_uncertain_points, dim=1)[1]
    # generator-side check: the kept set is separated from the dropped points
    mag = (-point_uncertainties[:, 0, :]).sort(dim=1).values
    if float((mag[:, num_uncertain_points] - mag[:, num_uncertain_points - 1]).min()) < TOPK_GAP:
        raise Retry("top-k gap below 1e-3")
    _kept.append(idx.clone())
    shift = num_sampled * torch.arange(num_boxes, dtype=torch.long, device=coarse_logits.device)
    idx = idx + shift[:, None]
    point_coords = point_coords.view(-1, 2)[idx.view(-1), :].view(num_boxes, num_uncertain_points, 2)
    if num_random_points > 0:
        point_coords = torch.cat(
            [point_coords, torch.rand(num_boxes, num_random_points, 2, device=coarse_logits.device)], dim=1)
    return point_coords


def import_reference(ref_root):
    install_weaksup_stubs()
    pf = sys.modules["detectron2.projects.point_rend.point_features"]
    pf.point_sample = point_sample
    pf.get_uncertain_point_coords_with_randomness = get_uncertain_point_coords_with_randomness
    sys.path.insert(0, ref_root)
    for pkg in ("mask2former", "mask2former.modeling", "mask2former.utils", "mask2former_video",
                "mask2former_video.modeling", "mask2former_video.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
        sys.modules[pkg] = m
    ref = types.SimpleNamespace(
        matcher=importlib.import_module("mask2former.modeling.matcher"),
        criterion=importlib.import_module("mask2former.modeling.criterion"),
        vmatcher=importlib.import_module("mask2former_video.modeling.matcher"),
        vcriterion=importlib.import_module("mask2former_video.modeling.criterion"))
    # The reference's VideoHungarianMatcher cannot run as checked in: its module calls batch_sigmoid_ce_loss_jit
    # (mask2former_video/modeling/matcher.py:570) without defining it, and the module's batch_dice_loss (:21-35)
    # has no sigmoid (the box-supervised matchers of that file hand it probabilities, :43-54), while this matcher
    # hands it logits (:573).  The video matcher is therefore run with the image matcher's two cost functions
    # (mask2former/modeling/matcher.py:105-158): sigmoid-CE and dice on sigmoid(x), over the T K samples.
    ref.vmatcher.batch_sigmoid_ce_loss_jit = ref.matcher.batch_sigmoid_ce_loss_jit
    ref.vmatcher.batch_dice_loss_jit = ref.matcher.batch_dice_loss_jit
    return ref


def make_targets(gen, case):
    """Per image: labels and bool masks (G, [T,] Ht, Wt): one ellipse per target (drifting over the frames)."""
    out = []
    T = case["T"]
    for b, (G, (Ht, Wt)) in enumerate(zip(case["G"], case["sizes"])):
        yy, xx = torch.meshgrid(torch.arange(Ht).float(), torch.arange(Wt).float(), indexing="ij")
        masks = torch.zeros((G, max(T, 1), Ht, Wt), dtype=torch.bool)
        for g in range(G):
            cy, cx = float(torch.rand(1, generator=gen)) * Ht, float(torch.rand(1, generator=gen)) * Wt
            ry, rx = (0.12 + 0.2 * float(torch.rand(1, generator=gen))) * Ht, \
                (0.12 + 0.2 * float(torch.rand(1, generator=gen))) * Wt
            for t in range(max(T, 1)):
                masks[g, t] = ((yy - cy - 2 * t) / ry) ** 2 + ((xx - cx + 3 * t) / rx) ** 2 <= 1.0
        labels = torch.randint(0, CLASSES, (G,), generator=gen)
        out.append({"labels": labels, "masks": masks if T else masks[:, 0]})
    return out


def make_masks(gen, case, targets):
    """int16 logits * MASK_SCALE: noise, plus a low-resolution copy of a target on some queries."""
    B, Q, T, H, W = (case[k] for k in ("B", "Q", "T", "H", "W"))
    shape = (B, Q, T, H, W) if T else (B, Q, H, W)
    k = (torch.randn(shape, generator=gen) * 3 * MASK_SCALE).round().clamp(-12 * MASK_SCALE, 12 * MASK_SCALE)
    for b, t in enumerate(targets):
        for g in range(t["masks"].shape[0]):
            q = int(torch.randint(0, Q, (1,), generator=gen))
            m = t["masks"][g].float()
            m = m[None] if T else m[None, None]
            low = F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)[0]
            k[b, q] += (low if T else low[0]) * 5 * MASK_SCALE
    return k.round().to(torch.int16)


def run_case(ref_matcher, ref_crit_cls, ref_matcher_cls, case, seed, video):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    B, Q = case["B"], case["Q"]
    targets = make_targets(gen, case)
    matcher = ref_matcher_cls(cost_class=WEIGHTS["loss_ce"], cost_mask=WEIGHTS["loss_mask"],
                              cost_dice=WEIGHTS["loss_dice"], num_points=NUM_POINTS)
    args = (CLASSES,)
    kw = dict(matcher=matcher, weight_dict=WEIGHTS, eos_coef=0.1, losses=["labels", "masks"],
              num_points=NUM_POINTS, oversample_ratio=OVERSAMPLE, importance_sample_ratio=IMPORTANCE)
    if not video:
        kw["mask_target_type"] = "mask"
    crit = ref_crit_cls(*args, **kw)
    res = {"state_keys": np.array(sorted(crit.state_dict().keys())), "repr": np.array(repr(crit))}
    for b, t in enumerate(targets):
        res[f"labels{b}"] = t["labels"].numpy()
        res[f"masks{b}"] = np.packbits(t["masks"].numpy(), axis=-1)
        res[f"size{b}"] = np.array(t["masks"].shape[-2:], np.int64)

    calls, draws = [], []
    lsa = ref_matcher.linear_sum_assignment
    pert = np.random.default_rng(5)

    def spy(C):
        r = lsa(C)
        c = np.asarray(C, dtype=np.float64)
        for _ in range(16):
            p = c * (1 + 1e-5 * pert.choice([-1.0, 1.0], c.shape))
            if not all(np.array_equal(x, y) for x, y in zip(lsa(p), r)):
                raise Retry("assignment is not stable")
        calls.append(r)
        return r

    rand = torch.rand

    def rec_rand(*a, **k):
        v = rand(*a, **k)
        draws.append(v.clone())
        return v

    heads = []
    for hd in range(N_AUX + 1):
        lg = (torch.randn(B, Q, CLASSES + 1, generator=gen) * 2).requires_grad_()
        mq = make_masks(gen, case, targets)
        mk = (mq.float() / MASK_SCALE).requires_grad_()
        heads.append({"pred_logits": lg, "pred_masks": mk, "q": mq})
    outputs = {k: v for k, v in heads[-1].items() if k != "q"}
    outputs["aux_outputs"] = [{k: v for k, v in h.items() if k != "q"} for h in heads[:-1]]
    _kept.clear()
    ref_matcher.linear_sum_assignment = spy
    torch.rand = rec_rand
    try:
        losses = crit(outputs, targets)
    finally:
        torch.rand = rand
        ref_matcher.linear_sum_assignment = lsa
    total = sum(losses[k] * WEIGHTS[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k in losses)
    total.sum().backward()
    n_rand = NUM_POINTS - int(IMPORTANCE * NUM_POINTS)
    per_head = B + 1 + (1 if n_rand else 0)
    order = [N_AUX] + list(range(N_AUX))          # the criterion's head order: main, aux 0, aux 1
    assert len(calls) == B * len(order) and len(draws) == per_head * len(order) and len(_kept) == len(order)
    for c, hd in enumerate(order):
        d = draws[c * per_head:(c + 1) * per_head]
        assert all(x.shape == (1, NUM_POINTS, 2) for x in d[:B])
        res[f"match{hd}"] = torch.cat(d[:B]).numpy()                 # (B, K, 2): one draw per image, in order
        res[f"oversample{hd}"] = d[B].numpy()
        assert d[B].shape[1] == int(NUM_POINTS * OVERSAMPLE)
        if n_rand:
            res[f"random{hd}"] = d[B + 1].numpy()
            assert d[B + 1].shape[1:] == (n_rand, 2)
        res[f"kept{hd}"] = _kept[c].sort(dim=1).values.numpy()
        for b in range(B):
            i, j = calls[c * B + b]
            res[f"idx{hd}_{b}"] = np.stack([i, j]).astype(np.int64)
    for hd, h in enumerate(heads):
        res[f"logits{hd}"] = h["pred_logits"].detach().numpy()
        res[f"pmasks{hd}"] = h["q"].numpy()
        res[f"glogits{hd}"] = h["pred_logits"].grad.numpy()
        res[f"gmasks{hd}"] = h["pred_masks"].grad.numpy()
    for k, v in losses.items():
        res[k] = np.float64(v.sum().item())
    res["loss_keys"] = np.array(sorted(losses.keys()))
    return res


def gen_all(ref, out_dir):
    res = {"n_aux": N_AUX, "classes": CLASSES, "num_points": NUM_POINTS, "oversample": OVERSAMPLE,
           "importance": IMPORTANCE, "mask_scale": MASK_SCALE, "weights": np.array([WEIGHTS[k] for k in LOSS_ORDER])}
    for name, case, video, mod_m, cls_m, cls_c in (
            ("img", IMAGE, False, ref.matcher, ref.matcher.HungarianMatcher, ref.criterion.SetCriterion),
            ("vid", VIDEO, True, ref.vmatcher, ref.vmatcher.VideoHungarianMatcher, ref.vcriterion.VideoSetCriterion)):
        for seed in range(2024, 2024 + 400):
            try:
                r = run_case(mod_m, cls_c, cls_m, case, seed, video)
                break
            except Retry as e:
                print(f"{name}: seed {seed}: {e}")
        else:
            raise AssertionError("no seed satisfies the generator's checks")
        print(f"{name}: seed {seed}")
        res[f"{name}_seed"] = seed
        for k in ("B", "Q", "T", "H", "W"):
            res[f"{name}_{k}"] = case[k]
        res.update({f"{name}_{k}": v for k, v in r.items()})
    path = os.path.join(out_dir, "mask_criterion.npz")
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
