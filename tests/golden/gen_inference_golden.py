"""Generate tests/golden/inference.npz (+ inference_semseg_<case><image>.npz) by running the REFERENCE inference
heads on the CPU (nothing of the reference is copied: the fixtures hold inputs and results only).

    python tests/golden/gen_inference_golden.py --ref <reference checkout>

``mask2former.maskformer_model`` is imported in place with the stand-ins of gen_criterion_golden, and the three
``MaskFormer.*_inference`` methods (maskformer_model.py:509-624) are called unbound on a SimpleNamespace self, fed by
the F.interpolate + sem_seg_postprocess chain of :337-364.  ``sem_seg_postprocess`` belongs to detectron2; it is a
crop plus a bilinear interpolate and is restated here, as are minimal ``Instances`` / ``Boxes``.

The (K, H, W) semantic scores dominate the size, so each image's go to a file of their own (every committed file
stays below 1 MiB); everything else is in inference.npz.  The archives are written with fixed timestamps and sorted
keys, so a rerun reproduces them byte for byte.

Besides the reference's results the fixture stores an fp64 evaluation with per-pixel ambiguity maps (where fp32
rounding may legitimately flip a discrete result), and the generator asserts that the cases reach every panoptic
event and stay clear of the thresholds (see ``run_case``).  If a seed fails an assert, change the seed, not the caps.
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

OBJECT_MASK_THRESHOLD = 0.8
OVERLAP_THRESHOLD = 0.8
REL = 1e-5            # ambiguity: relative margins below this
AMB_CAP = 0.005       # at most this fraction of an image's pixels may be ambiguous
RATIO_MARGIN = 0.02   # every candidate's mask_area / original_area keeps this distance from OVERLAP_THRESHOLD

CASES = {
    # things 0..79 of 133 classes; neither Q nor K is a multiple of 32; image 1 keeps no query
    "coco": dict(seed=11, Q=100, K=133, things=80, topk=100, logit_hw=(8, 12), padded=(32, 48),
                 image_sizes=[(32, 48), (30, 41)], output_sizes=[(32, 48), (23, 31)], events=[True, False],
                 roles=[3, 17, 18, 40, 41, 77, 90], stuff=(100, 90), thing=(5, 7)),
    # non-integer upscale by the second stage
    "tiny": dict(seed=5, Q=20, K=6, things=3, topk=30, logit_hw=(16, 24), padded=(64, 96),
                 image_sizes=[(60, 90)], output_sizes=[(97, 131)], events=[True], after=True,
                 roles=[1, 4, 5, 9, 12, 15, 18], stuff=(4, 5), thing=(1, 2)),
}


class _Instances:
    def __init__(self, image_size):
        self.image_size = image_size


class _Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


def sem_seg_postprocess(result, img_size, output_height, output_width):
    """detectron2.modeling.postprocessing.sem_seg_postprocess: crop to the image, resize to the output."""
    result = result[:, :img_size[0], :img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


def make_inputs(c):
    """Class and mask logits with a planted panoptic story on the 'event' images:
    roles[0], roles[1]  kept, same stuff class, disjoint stripes          -> merge into one segment
    roles[2], roles[3]  kept, same thing class, disjoint stripes          -> two segments
    roles[4]            kept (score ~0.9), covers stripes 2-4, wins on 4  -> dropped by overlap_threshold
    roles[5]            kept, mask negative everywhere                    -> original_area == 0
    roles[6]            non-void label with score ~0.4                    -> dropped by object_mask_threshold
    every other query predicts void."""
    g = torch.Generator().manual_seed(c["seed"])
    Q, K, (h, w) = c["Q"], c["K"], c["logit_hw"]
    B = len(c["image_sizes"])
    cls = torch.randn(B, Q, K + 1, generator=g) * 0.1
    masks = torch.randn(B, Q, h, w, generator=g) * 3
    unit = w // 12
    stripe = torch.repeat_interleave(torch.arange(5), torch.tensor([2, 2, 3, 3, 2]) * unit)[None, :].expand(h, w)
    logk = float(np.log(K))
    for b, ev in enumerate(c["events"]):
        if not ev:
            cls[b, :, K] += 10
            continue
        cls[b, :, K] += 10
        r = c["roles"]
        plan = [(r[0], c["stuff"][0], 12.0, [0]), (r[1], c["stuff"][0], 12.0, [1]), (r[2], c["thing"][0], 12.0, [2]),
                (r[3], c["thing"][0], 12.0, [3]), (r[4], c["stuff"][1], float(np.log(9.0)) + logk, [2, 3, 4]),
                (r[5], c["thing"][1], 12.0, None), (r[6], c["thing"][1], float(np.log(0.4 / 0.6)) + logk, [0, 1])]
        for q, klass, logit, stripes in plan:
            cls[b, q, K] -= 10
            cls[b, q, klass] += logit
            noise = torch.randn(h, w, generator=g)
            if stripes is None:
                masks[b, q] = -(noise.abs() * 3) - 0.5
            else:
                on = torch.zeros(h, w, dtype=torch.bool)
                for s in stripes:
                    on |= stripe == s
                masks[b, q] = torch.where(on, torch.tensor(4.0), torch.tensor(-4.0)) + noise
    return cls, masks


def fp64_eval(cls, full, K):
    """fp64 restatement on full-resolution logits (Q, H, W) float64: counters, ambiguity maps, runner-ups."""
    probs = F.softmax(cls.double(), dim=-1)
    scores, labels = probs.max(-1)
    keep = labels.ne(K) & (scores > OBJECT_MASK_THRESHOLD)
    kidx = keep.nonzero().flatten()
    sig = full.sigmoid()
    amax = full.abs()[full.isfinite()].max()                            # infinite logits do not set the scale
    near_zero = full.abs() < REL * amax                                  # (Q, H, W): `> 0` / `>= 0.5` may flip
    sem = torch.einsum("qc,qhw->chw", probs[:, :-1], sig)
    top2 = sem.topk(2, dim=0)
    out = {"sem_amb": (top2.values[0] - top2.values[1]) < REL * top2.values[0], "sem_alt": top2.indices[1],
           "thr_amb": near_zero, "n_keep": len(kidx), "kidx": kidx}
    H, W = full.shape[-2:]
    if len(kidx) == 0:
        out.update(pan_amb=torch.zeros(H, W, dtype=torch.bool), counters=torch.zeros(0, 3, dtype=torch.int64),
                   classes=torch.zeros(0, dtype=torch.int64), pan_alt=torch.zeros(H, W, dtype=torch.int64))
        return out
    p = scores[kidx].view(-1, 1, 1) * sig[kidx]
    if len(kidx) > 1:
        t2 = p.topk(2, dim=0)
        margin = (t2.values[0] - t2.values[1]) < REL * t2.values[0]
        second = t2.indices[1]
    else:
        margin = torch.zeros(H, W, dtype=torch.bool)
        second = torch.zeros(H, W, dtype=torch.int64)
    win = p.argmax(0)
    above = sig[kidx] >= 0.5
    inside = above.gather(0, win[None])[0]
    out["pan_amb"] = margin | near_zero[kidx].gather(0, win[None])[0] | near_zero[kidx].gather(0, second[None])[0]
    out["counters"] = torch.stack([torch.bincount(win.flatten(), minlength=len(kidx)), above.flatten(1).sum(1),
                                   torch.bincount(win[inside], minlength=len(kidx))], 1)
    out["classes"] = labels[kidx]
    out["winner"], out["second"], out["second_in"] = win, second, above.gather(0, second[None])[0]
    out["inside"] = inside
    out["score_drop"] = int((labels.ne(K) & ~(scores > OBJECT_MASK_THRESHOLD)).sum())
    return out


def merge_loop(classes, counters, things):
    """The segment loop of :541-569 over counters -> (lut, segments_info, events)."""
    lut, info, memory, cur = [0] * (len(classes) + 1), [], {}, 0
    ev = {"overlap_drop": 0, "merge": 0, "no_original_area": 0, "ratios": []}
    for k, (pc, (ma, oa, it)) in enumerate(zip(classes, counters)):
        isthing = pc < things
        ev["no_original_area"] += oa == 0
        if ma > 0 and oa > 0 and it > 0:
            ev["ratios"].append(ma / oa)
            if ma / oa < OVERLAP_THRESHOLD:
                ev["overlap_drop"] += 1
                continue
            if not isthing:
                if pc in memory:
                    lut[k + 1] = memory[pc]
                    ev["merge"] += 1
                    continue
                memory[pc] = cur + 1
            cur += 1
            lut[k + 1] = cur
            info.append((cur, int(isthing), pc))
    return lut, info, ev


def run_case(ref, name, c):
    MaskFormer = ref.model.MaskFormer
    cls, masks = make_inputs(c)
    K, Q, things = c["K"], c["Q"], c["things"]
    fake = types.SimpleNamespace(
        sem_seg_head=types.SimpleNamespace(num_classes=K),
        metadata=types.SimpleNamespace(thing_dataset_id_to_contiguous_id={1000 + i: i for i in range(things)}),
        num_queries=Q, device=torch.device("cpu"), object_mask_threshold=OBJECT_MASK_THRESHOLD,
        overlap_threshold=OVERLAP_THRESHOLD, panoptic_on=True, test_topk_per_image=c["topk"])
    res = {f"{name}_pred_logits": cls.numpy(), f"{name}_pred_masks": masks.numpy(),
           f"{name}_meta": np.array([Q, K, things, c["topk"], *c["padded"]], dtype=np.int64),
           f"{name}_image_sizes": np.array(c["image_sizes"], dtype=np.int64),
           f"{name}_output_sizes": np.array(c["output_sizes"], dtype=np.int64),
           f"{name}_thresholds": np.array([OBJECT_MASK_THRESHOLD, OVERLAP_THRESHOLD])}
    sem_files = {}
    up = F.interpolate(masks, size=c["padded"], mode="bilinear", align_corners=False)       # :337-342
    up64 = F.interpolate(masks.double(), size=c["padded"], mode="bilinear", align_corners=False)
    seen = {"score_drop": 0, "overlap_drop": 0, "merge": 0, "no_original_area": 0, "empty": 0}
    for b, (isz, osz) in enumerate(zip(c["image_sizes"], c["output_sizes"])):
        key = f"{name}{b}"
        full = sem_seg_postprocess(up[b], isz, *osz)                                          # :355-357
        full64 = sem_seg_postprocess(up64[b], isz, *osz)
        sem = MaskFormer.semantic_inference(fake, cls[b], full)
        pan, info = MaskFormer.panoptic_inference(fake, cls[b], full)
        inst = MaskFormer.instance_inference(fake, cls[b], full)
        # the semantic head without postprocessing before inference (:362-364): scores resized afterwards
        sem_files[key] = {"sem_seg": sem.numpy()}
        if c.get("after"):
            sem_after = sem_seg_postprocess(MaskFormer.semantic_inference(fake, cls[b], up[b]), isz, *osz)
            sem_files[key]["sem_seg_after"] = sem_after.numpy()

        # which query each instance came from: the same topk on the same scores (:578-584)
        sc = F.softmax(cls[b], dim=-1)[:, :-1]
        tk_s, tk_i = sc.flatten(0, 1).topk(c["topk"], sorted=False)
        lab = tk_i % K
        keep_t = lab < things
        assert torch.equal(lab[keep_t], inst.pred_classes)
        qidx = (tk_i // K)[keep_t]
        assert torch.equal((full[qidx] > 0).float(), inst.pred_masks)

        e = fp64_eval(cls[b], full64, K)
        lut, info64, ev = merge_loop(e["classes"].tolist(), e["counters"].tolist(), things)
        assert info64 == [(s["id"], int(s["isthing"]), s["category_id"]) for s in info], (key, info64, info)
        npix = osz[0] * osz[1]
        for m in ("sem_amb", "pan_amb"):
            assert e[m].sum().item() <= AMB_CAP * npix, (key, m, e[m].sum().item())
        assert e["thr_amb"][qidx].flatten(1).sum(1).max().item() <= AMB_CAP * npix, key
        for r in ev["ratios"]:
            assert abs(r - OVERLAP_THRESHOLD) >= RATIO_MARGIN, (key, r)
        if e["n_keep"]:
            lut_t = torch.tensor(lut)
            expect = lut_t[e["winner"] + 1] * e["inside"]
            assert torch.equal(expect[~e["pan_amb"]].int(), pan[~e["pan_amb"]]), key
            pan_alt = lut_t[e["second"] + 1] * e["second_in"]
            pan_top = lut_t[e["winner"] + 1]
            seen["score_drop"] += e["score_drop"]
        else:
            assert pan.abs().sum() == 0 and info == []
            seen["empty"] += 1
            pan_alt = pan_top = e["pan_alt"]
        for k in ("overlap_drop", "merge", "no_original_area"):
            seen[k] += ev[k]
        # topk(sorted=False) fixes no order and the result does not name its query: tests order instances by
        # (class, score), which is unambiguous when scores of one class are well apart (or exactly zero)
        fin, fcl = inst.scores.numpy().astype(np.float64), inst.pred_classes.numpy()
        o = np.lexsort((fin, fcl))
        fin, fcl = fin[o], fcl[o]
        same = fcl[1:] == fcl[:-1]
        assert np.all(~same | (np.diff(fin) > 1e-4 * fin[1:]) | (fin[1:] == 0)), (key, "instance scores too close")

        res[f"{key}_panoptic_seg"] = pan.numpy()
        res[f"{key}_segments_info"] = np.array([(s["id"], int(s["isthing"]), s["category_id"]) for s in info],
                                               dtype=np.int64).reshape(-1, 3)
        res[f"{key}_sem_labels"] = sem.argmax(0).numpy().astype(np.int16)
        res[f"{key}_inst_masks"] = np.packbits(inst.pred_masks.numpy().astype(bool), axis=-1)
        res[f"{key}_inst_scores"] = inst.scores.numpy()
        res[f"{key}_inst_classes"] = inst.pred_classes.numpy()
        res[f"{key}_inst_queries"] = qidx.numpy()
        assert inst.pred_boxes.tensor.abs().sum() == 0 and tuple(inst.image_size) == tuple(osz)
        res[f"{key}_counters"] = e["counters"].numpy().astype(np.int64).reshape(-1, 3)
        res[f"{key}_keep_classes"] = e["classes"].numpy()
        res[f"{key}_keep_queries"] = e["kidx"].numpy()
        res[f"{key}_pan_amb"] = np.packbits(e["pan_amb"].numpy(), axis=-1)
        res[f"{key}_pan_alt"] = pan_alt.numpy().astype(np.int32)   # the runner-up's segment, were it to win
        res[f"{key}_pan_top"] = pan_top.numpy().astype(np.int32)   # the winner's segment, whatever its own sigmoid
        res[f"{key}_sem_amb"] = np.packbits(e["sem_amb"].numpy(), axis=-1)
        res[f"{key}_sem_alt"] = e["sem_alt"].numpy().astype(np.int16)
        res[f"{key}_thr_amb"] = np.packbits(e["thr_amb"].numpy(), axis=-1)   # (Q, Ho, ceil(Wo / 8))
    return res, sem_files, seen


def write_npz(path, arrays):
    """np.load-compatible archive with sorted keys and a fixed timestamp (byte-identical on a rerun)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(1)   # one thread: the reference's fp32 reductions do not depend on the host's core count
    from gen_criterion_golden import import_reference
    ref = import_reference(a.ref)
    ref.model.Instances = _Instances
    ref.model.Boxes = _Boxes
    res, total = {}, {}
    for name, c in CASES.items():
        r, sem_files, seen = run_case(ref, name, c)
        res.update(r)
        for key, arrays in sem_files.items():
            write_npz(os.path.join(a.out, f"inference_semseg_{key}.npz"), arrays)
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        # every event image plants every event
        assert all(seen[k] >= sum(c["events"]) for k in ("score_drop", "overlap_drop", "merge", "no_original_area")), \
            (name, seen)
    assert total["empty"] >= 1, total
    write_npz(os.path.join(a.out, "inference.npz"), res)
    print("wrote inference.npz and", sum(len(c["image_sizes"]) for c in CASES.values()), "semseg files;", total)


if __name__ == "__main__":
    main()
