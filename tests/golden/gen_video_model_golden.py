"""Generate tests/golden/video_model.npz by running the REFERENCE video meta-architecture's host code on the CPU
(nothing of the reference is copied: the fixture holds inputs and results only).

    python tests/golden/gen_video_model_golden.py --ref <reference checkout>

``mask2former_video.video_maskformer_model`` is imported in place with the stand-ins of
gen_criterion_golden.install_weaksup_stubs, plus a restated ``BitMasks.get_bounding_boxes`` and a minimal
``Instances`` (both belong to detectron2).  ``VideoMaskFormer.inference_video`` (:651-694, fed by the F.interpolate of
the eval branch :372-393), ``.prepare_weaksup_targets`` (:395-620) and ``.prepare_targets`` (:622-649) are called
unbound on a SimpleNamespace self, as gen_inference_golden.py does.

Inference cases: Q = 12, K = 5, T = 3 (``INFER``); mask logits are multiples of 1/16 stored as int16.  Asserted for
the reference alone: the top-10 set is unchanged under a 1e-5 relative perturbation of the scores; (class, score)
pairs are far enough apart to pair entries unambiguously; one query is selected under two classes; an fp64 evaluation
marks a pixel ambiguous when its |logit| is below REL of its mask's max |logit| (REL, AMB_CAP of
gen_inference_golden.py), and at most AMB_CAP of any case's pixels are.

Target cases: B = 2 clips, T = 3, D = 8; frames 44 x 60 (clip 0) and 40 x 52 (clip 1), both padded to 64 x 64.
Fractional boxes; one instance is absent from the middle frame (zero box, id -1), one from every frame (dropped by
``valid_idx``), one touches the frame edge.  Features are multiples of 1/16 stored as int8, so the stride-4 resize
(weights exactly 1/2) is exact in fp32.  The Lab images are captured from the reference's ``color.rgb2lab`` calls, the
resized features from its ``get_instance_temporal_pairs`` calls.  The mined rows keep the ambiguity assertion of
gen_video_criterion_golden.py (at most 10 % ambiguous).

The archive is written with fixed timestamps and sorted keys: a rerun reproduces it byte for byte.  If a seed fails
an assert, change the seed, not the caps.
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
from gen_inference_golden import AMB_CAP, REL, write_npz  # noqa: E402

Q, K, T, TOPK = 12, 5, 3, 10
MASK_SCALE = 16          # mask logits are stored as int16 = logit * 16
FEAT_SCALE = 16          # features as int8 = feature * 16
INFER = {
    "a": dict(seed=3, logit_hw=(8, 12), padded=(32, 48), image=(30, 41), output=(23, 31)),   # two stages
    "b": dict(seed=3, logit_hw=(8, 12), padded=(32, 48), image=(30, 41), output=(30, 41)),   # one stage
    "c": dict(seed=3, logit_hw=(8, 12), padded=(32, 48), image=(30, 41), output=(45, 62)),   # second stage upscales
    "d": dict(seed=4, logit_hw=(40, 56), padded=(40, 56), image=(38, 53), output=(7, 9)),    # strong downscale
}
D = 8
SIZES = [(44, 60), (40, 52)]
# per clip and instance: label, and per frame (id, x0, y0, x1, y1); id -1 = absent (zero box)
CLIPS = [
    [(1, [(7, 5.3, 4.7, 30.2, 25.9), (7, 7.6, 6.1, 32.5, 27.2), (7, 9.2, 8.4, 33.8, 29.6)]),
     (4, [(3, 33.4, 2.2, 52.7, 17.5), (-1, 0, 0, 0, 0), (3, 35.1, 5.8, 55.3, 21.4)]),
     (0, [(-1, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (-1, 0, 0, 0, 0)]),
     (2, [(9, 40.5, 20.2, 59.9, 43.8), (9, 38.3, 22.6, 59.9, 43.8), (9, 41.7, 24.1, 59.9, 43.8)])],
    [(3, [(1, 10.8, 6.4, 34.1, 30.3), (1, 12.2, 7.9, 36.6, 31.5), (1, 13.5, 9.3, 38.9, 33.7)]),
     (0, [(5, 0.0, 18.6, 21.4, 39.9), (5, 0.0, 17.2, 23.8, 39.9), (5, 0.0, 16.5, 25.1, 39.9)])],
]


# ---------------------------------------------------------------------------------------------------------------
# detectron2 stand-ins
# ---------------------------------------------------------------------------------------------------------------
class _Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


class _BitMasks:
    def __init__(self, tensor):
        self.tensor = tensor

    def get_bounding_boxes(self):
        """detectron2 BitMasks.get_bounding_boxes: [x_min, y_min, x_max + 1, y_max + 1], zeros for an empty mask."""
        boxes = torch.zeros(self.tensor.shape[0], 4, dtype=torch.float32)
        x_any = torch.any(self.tensor, dim=1)
        y_any = torch.any(self.tensor, dim=2)
        for idx in range(self.tensor.shape[0]):
            x = torch.where(x_any[idx, :])[0]
            y = torch.where(y_any[idx, :])[0]
            if len(x) > 0 and len(y) > 0:
                boxes[idx, :] = torch.as_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1], dtype=torch.float32)
        return _Boxes(boxes)


class _Instances:
    def __init__(self, image_size, boxes, classes, ids, masks):
        self.image_size = image_size
        self.gt_boxes, self.gt_classes, self.gt_ids, self.gt_masks = _Boxes(boxes), classes, ids, _BitMasks(masks)

    def __len__(self):
        return self.gt_classes.shape[0]

    def to(self, device):
        return self


def import_reference(ref_root):
    install_weaksup_stubs()
    sys.path.insert(0, ref_root)
    for pkg in ("mask2former", "mask2former.modeling", "mask2former.utils", "mask2former_video",
                "mask2former_video.modeling", "mask2former_video.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
        sys.modules[pkg] = m
    model = importlib.import_module("mask2former_video.video_maskformer_model")
    model.BitMasks = _BitMasks
    return model


# ---------------------------------------------------------------------------------------------------------------
# inference
# ---------------------------------------------------------------------------------------------------------------
def chain(x, padded, image, output):
    """The eval branch's resize chain (:378-383, :661-664) on (N, T, h, w)."""
    x = F.interpolate(x, size=padded, mode="bilinear", align_corners=False)
    x = x[:, :, :image[0], :image[1]]
    return F.interpolate(x, size=output, mode="bilinear", align_corners=False)


def run_inference(model, name, c):
    g = torch.Generator().manual_seed(c["seed"])
    h, w = c["logit_hw"]
    cls = torch.randn(Q, K + 1, generator=g)
    cls[4, 1] += 4.0          # query 4 is selected under two classes
    cls[4, 3] += 3.8
    coarse = torch.randn(Q, T, (h + 3) // 4, (w + 3) // 4, generator=g).repeat_interleave(4, 2) \
        .repeat_interleave(4, 3)[..., :h, :w]
    mq = ((coarse * 3 + torch.randn(Q, T, h, w, generator=g)) * MASK_SCALE).round().clamp(-200, 200).to(torch.int16)
    masks = mq.float() / MASK_SCALE
    fake = types.SimpleNamespace(sem_seg_head=types.SimpleNamespace(num_classes=K), num_queries=Q,
                                 device=torch.device("cpu"))
    up = F.interpolate(masks, size=c["padded"], mode="bilinear", align_corners=False)            # :378-383
    out = model.VideoMaskFormer.inference_video(fake, cls, up, c["image"], *c["output"], None)
    assert tuple(out["image_size"]) == tuple(c["output"]) and len(out["pred_masks"]) == TOPK

    scores = F.softmax(cls, dim=-1)[:, :-1].flatten()
    tk_s, tk_i = scores.topk(TOPK, sorted=False)
    assert tk_s.tolist() == out["pred_scores"] and (tk_i % K).tolist() == out["pred_labels"]
    qidx = tk_i // K
    assert len(set(qidx.tolist())) < TOPK, "no query is selected under two classes: change the seed"
    rng = np.random.default_rng(5)
    base = set(tk_i.tolist())
    for _ in range(16):
        p = scores.double() * (1 + 1e-5 * torch.from_numpy(rng.choice([-1.0, 1.0], scores.shape)))
        assert set(p.topk(TOPK).indices.tolist()) == base, "top-k is not stable: change the seed"
    lab, sc = np.array(out["pred_labels"]), np.array(out["pred_scores"], dtype=np.float64)
    o = np.lexsort((sc, lab))
    same = lab[o][1:] == lab[o][:-1]
    assert np.all(~same | (np.diff(sc[o]) > 1e-4 * sc[o][1:])), "scores of one class too close: change the seed"

    pm = torch.stack(out["pred_masks"])                                                           # (10, T, Ho, Wo)
    full64 = chain(masks.double()[qidx], c["padded"], c["image"], c["output"])
    amb = full64.abs() < REL * full64.abs().flatten(1).amax(1).view(-1, 1, 1, 1)
    npix = T * c["output"][0] * c["output"][1]
    assert amb.flatten(1).sum(1).max().item() <= AMB_CAP * npix, (name, "too many ambiguous pixels")
    assert torch.equal((full64 > 0)[~amb], pm[~amb]), name
    return {f"{name}_pred_logits": cls.numpy(), f"{name}_pred_masks": mq.numpy(),
            f"{name}_geometry": np.array([*c["padded"], *c["image"], *c["output"]], dtype=np.int64),
            f"{name}_scores": np.array(out["pred_scores"], dtype=np.float32),
            f"{name}_labels": np.array(out["pred_labels"], dtype=np.int64),
            f"{name}_queries": qidx.numpy(),
            f"{name}_masks": np.packbits(pm.numpy(), axis=-1),
            f"{name}_amb": np.packbits(amb.numpy(), axis=-1)}


# ---------------------------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------------------------
def make_clip(gen, b):
    Hf, Wf = SIZES[b]
    frames, images = [], []
    G = len(CLIPS[b])
    for t in range(T):
        yy, xx = torch.meshgrid(torch.arange(Hf), torch.arange(Wf), indexing="ij")
        base = torch.stack([(xx * 3 + 11 * t) % 256, (yy * 3) % 256, ((xx + yy) * 2) % 256]).float()
        blocks = (torch.rand(3, Hf // 8 + 1, Wf // 8 + 1, generator=gen) * 255).repeat_interleave(8, 1) \
            .repeat_interleave(8, 2)[:, :Hf, :Wf]
        region = (torch.rand(1, Hf // 16 + 1, Wf // 16 + 1, generator=gen) < 0.5).repeat_interleave(16, 1) \
            .repeat_interleave(16, 2)[:, :Hf, :Wf]
        img = torch.where(region, base * 0.5, blocks)
        images.append((img + torch.randint(-3, 4, (3, Hf, Wf), generator=gen)).clamp(0, 255).to(torch.uint8))
        boxes = torch.tensor([CLIPS[b][i][1][t][1:] for i in range(G)], dtype=torch.float32)
        ids = torch.tensor([CLIPS[b][i][1][t][0] for i in range(G)], dtype=torch.int64)
        masks = torch.zeros(G, Hf, Wf, dtype=torch.bool)
        for i in range(G):
            if ids[i] < 0:
                continue
            x0, y0, x1, y1 = (int(v) for v in boxes[i])
            blob = torch.rand(y1 + 1 - y0, x1 + 1 - x0, generator=gen) < 0.7
            masks[i, y0:y1 + 1, x0:x1 + 1] = blob[:Hf - y0, :Wf - x0]
        classes = torch.tensor([CLIPS[b][i][0] for i in range(G)], dtype=torch.int64)
        frames.append(_Instances((Hf, Wf), boxes, classes, ids, masks))
    # smooth field + noise: neighbouring pixels are similar but distinct
    coarse = torch.randn(T, D, Hf // 8 + 1, Wf // 8 + 1, generator=gen).repeat_interleave(8, 2) \
        .repeat_interleave(8, 3)[:, :, :Hf, :Wf]
    feats_q = ((coarse + torch.randn(T, D, Hf, Wf, generator=gen)) * FEAT_SCALE).round().clamp(-127, 127)
    return frames, images, feats_q.to(torch.int8)


def run_targets(model):
    gen = torch.Generator().manual_seed(77)
    B = len(CLIPS)
    clips = [make_clip(gen, b) for b in range(B)]
    targets = [{"instances": c[0]} for c in clips]
    org_images = [img for c in clips for img in c[1]]
    feats = [[(c[2][t].float() / FEAT_SCALE)[None] for t in range(T)] for c in clips]
    fake = types.SimpleNamespace(temporal_pairwise=True, num_frames=T, size_divisibility=32, mask_out_stride=4,
                                 pairwise_size=3, pairwise_dilation=2, temporal_k=1, device=torch.device("cpu"))
    labs, calls = [], []
    rgb2lab = model.color.rgb2lab
    mine = model.get_instance_temporal_pairs

    def lab_spy(img):
        r = rgb2lab(img)
        labs.append(np.asarray(r))
        return r

    def mine_spy(f, boxes, k=1):
        calls.append(f)                 # the slice keeps its clip's storage alive: storages stay distinct
        return mine(f, boxes, k=k)

    model.color = types.SimpleNamespace(rgb2lab=lab_spy)
    model.get_instance_temporal_pairs = mine_spy
    try:
        out = model.VideoMaskFormer.prepare_weaksup_targets(fake, targets, org_images, feats)
    finally:
        model.color = types.SimpleNamespace(rgb2lab=rgb2lab)
        model.get_instance_temporal_pairs = mine
    plain = model.VideoMaskFormer.prepare_targets(
        types.SimpleNamespace(num_frames=T, device=torch.device("cpu")), targets,
        types.SimpleNamespace(tensor=torch.zeros(B * T, 3, 64, 64)))
    assert len(labs) == B * T
    res = {"lab": np.stack(labs).transpose(0, 3, 1, 2).astype(np.float32)}                   # (B*T, 3, h, w)
    # resized features per clip, from the spied calls (grouped by storage, frame = storage offset)
    per_clip = {}
    for f in calls:
        key = f.untyped_storage().data_ptr()
        frame = f.storage_offset() // (f.shape[1] * f.shape[2] * f.shape[3])
        per_clip.setdefault(key, {}).update({frame: f[0], frame + 1: f[1]})
    per_clip = list(per_clip.values())
    assert len(per_clip) == B and all(sorted(p) == list(range(T)) for p in per_clip)
    rows = ambiguous = 0
    cdist_err, d64s = 0.0, []
    for b, (c, t_ref, t_plain) in enumerate(zip(clips, out, plain)):
        frames, images, feats_q = c
        G = len(frames[0])
        ids = torch.stack([f.gt_ids for f in frames], 1)
        valid = (ids != -1).any(-1)
        assert not valid.all() or b > 0, "clip 0 needs an instance absent from every frame"
        resized = torch.stack([per_clip[b][t] for t in range(T)])
        res[f"feats_ds{b}"] = resized.numpy()
        for t in range(T):
            res[f"image{b}_{t}"] = images[t].numpy()
        res[f"feats{b}"] = feats_q.numpy()
        res[f"boxes{b}"] = torch.stack([f.gt_boxes.tensor for f in frames], 1).numpy()        # (G, T, 4)
        res[f"in_ids{b}"] = ids.numpy()
        res[f"in_labels{b}"] = frames[0].gt_classes.numpy()
        res[f"in_masks{b}"] = np.packbits(torch.stack([f.gt_masks.tensor for f in frames], 1).numpy(), axis=-1)
        res[f"valid{b}"] = valid.numpy()
        for k in ("labels", "ids"):
            res[f"{k}{b}"] = t_ref[k].numpy()
            assert torch.equal(t_ref[k], t_plain[k])
        for k in ("box_masks", "masks"):
            res[f"{k}{b}"] = np.packbits(t_ref[k].numpy().astype(bool), axis=-1)
        res[f"full_masks{b}"] = np.packbits(t_plain["masks"].numpy().astype(bool), axis=-1)
        for k in ("left_bounds", "right_bounds", "top_bounds", "bottom_bounds"):
            res[f"{k}{b}"] = t_ref[k].numpy()
        sim = t_ref["color_similarities"]
        assert all(torch.equal(sim[0], s) for s in sim)
        res[f"sim{b}"] = sim[0].numpy()
        res[f"counters{b}"] = np.array([t_ref["total_temp_pair"].item(), t_ref["pos_temp_pair"].item()])
        # pairs of the valid instances, indexed as the returned targets are
        pairs = t_ref["temporal_pairs"]
        assert len(pairs) == G
        box4 = _BitMasks(t_ref["box_masks"].flatten(0, 1) > 0).get_bounding_boxes().tensor.long().view(-1, T, 4)
        res[f"box4{b}"] = box4.numpy()
        new = torch.cumsum(valid.long(), 0) - 1
        packed = []
        for i, per in enumerate(pairs):
            for t, (cur, nxt) in enumerate(per):
                if cur.shape[0] == 0:
                    continue
                assert valid[i], "an instance absent from every frame mined pairs"
                gi = int(new[i])
                packed.append(torch.cat([torch.full((len(cur), 1), gi), torch.full((len(cur), 1), t), cur.long(),
                                         nxt.long()], 1))
                cx0, cy0, cx1, cy1 = box4[gi, t].tolist()
                nx0, ny0, nx1, ny1 = box4[gi, t + 1].tolist()
                a = resized[t, :, cy0:cy1, cx0:cx1].flatten(1).t()
                nb = resized[t + 1, :, ny0:ny1, nx0:nx1].flatten(1).t()
                d64 = torch.cdist(a.double(), nb.double(), p=2)
                cdist_err = max(cdist_err, float((torch.cdist(a, nb, p=2).double() - d64).abs().max()))
                d64s.append(d64)
        res[f"pairs{b}"] = torch.cat(packed).numpy().astype(np.int32)                         # (P, 6) g t cx cy nx ny
    for d64 in d64s:
        ok = d64 <= d64.amin(1, keepdim=True) * (1 + 2.0 ** -9) + cdist_err
        rows += d64.shape[0]
        ambiguous += int((ok.sum(1) > 1).sum())
    print(f"mined rows {rows}, ambiguous {ambiguous}, cdist_abs_err {cdist_err:.3e}")
    assert rows > 0 and ambiguous <= 0.10 * rows, "too many ambiguous mined rows: change the seed"
    res["cdist_abs_err"] = np.float64(cdist_err)
    res["n_ambiguous"] = np.int64(ambiguous)
    res["target_meta"] = np.array([B, T, D, 64, 64, FEAT_SCALE], dtype=np.int64)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(1)   # one thread: the reference's fp32 reductions do not depend on the host's core count
    model = import_reference(a.ref)
    res = {"infer_meta": np.array([Q, K, T, TOPK, MASK_SCALE], dtype=np.int64)}
    for name, c in INFER.items():
        res.update(run_inference(model, name, c))
    res.update(run_targets(model))
    path = os.path.join(a.out, "video_model.npz")
    write_npz(path, res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
