"""Inference heads: the eval branch of the reference's ``MaskFormer.forward`` (maskformer_model.py:333-377) and
the three heads it calls, ``semantic_inference`` (:509-513), ``panoptic_inference`` (:515-571) and
``instance_inference`` (:573-624).

:class:`MaskFormerInference` takes the decoder's *low-resolution* ``pred_masks`` and never builds the
(B, Q, Hp, Wp) tensor the reference upsamples to.  The value of query q at an output pixel is defined by the chain

    F.interpolate((h, w) -> padded (Hp, Wp), bilinear) -> crop to the image (Hc, Wc)
        -> F.interpolate((Hc, Wc) -> (Ho, Wo), bilinear)        [sem_seg_postprocess; skipped when equal]

and is evaluated per pixel inside the HIP kernels of ``csrc/inference.hip`` (``m2f_infer_*`` in ``include/bm2f.h``).
Logits may be fp32, fp16 or bf16; they are converted to fp32 on load and everything after is fp32, i.e. for 16-bit
logits the result is the reference's on ``logits.float()``.

On a HIP tensor the module calls the kernels; on a CPU tensor it runs a plain-torch restatement of the same
definition, so the semantics are testable without a GPU.  The CPU path is not a fallback: a kernel error raises
``NativeError``.

The class softmax and ``topk(sorted=False)`` stay in torch (they are tiny).  The panoptic head copies its per-query
area counters to the host once per batch, where the reference synchronises three times per kept query.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _native
from .rle import _BYTES, _encode_device, rle_encode

_MAX_Q = 256
_MAX_K = 256
_INSTANCE_TILE = 1024


def _pair(s):
    return int(s[0]), int(s[1])


def _geometry(padded_size, image_sizes, output_sizes):
    """[(Hc, Wc, Ho, Wo)] per image, validated against the padded size."""
    Hp, Wp = _pair(padded_size)
    if output_sizes is None:
        output_sizes = image_sizes
    if len(output_sizes) != len(image_sizes):
        raise ValueError("output_sizes and image_sizes differ in length")
    geo = []
    for isz, osz in zip(image_sizes, output_sizes):
        (Hc, Wc), (Ho, Wo) = _pair(isz), _pair(osz if osz is not None else isz)
        if not (0 < Hc <= Hp and 0 < Wc <= Wp and Ho > 0 and Wo > 0):
            raise ValueError(f"image size {(Hc, Wc)} / output size {(Ho, Wo)} do not fit the padded size {(Hp, Wp)}")
        geo.append((Hc, Wc, Ho, Wo))
    return geo


def full_resolution_logits(mask_pred, padded_size, image_size, output_size=None):
    """The definition, in torch: (Q, h, w) logits -> (Q, Ho, Wo) fp32 (maskformer_model.py:337-342, :355-357)."""
    Hc, Wc = _pair(image_size)
    Ho, Wo = _pair(output_size) if output_size is not None else (Hc, Wc)
    m = mask_pred.float()
    m = F.interpolate(m[None], size=_pair(padded_size), mode="bilinear", align_corners=False)[0]
    m = m[:, :Hc, :Wc]
    if (Ho, Wo) != (Hc, Wc):
        m = F.interpolate(m[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0]
    return m


# -------------------------------------------------------------------------------------------------------------------
# host side of the panoptic head
# -------------------------------------------------------------------------------------------------------------------
def merge_segments(classes, counters, thing_classes, overlap_threshold):
    """The segment loop of panoptic_inference (:541-569) over per-query counters.

    classes: predicted class of each kept query; counters: rows [mask_area, original_area, intersection].
    Returns (lut, segments_info): lut[k + 1] is the segment id of kept query k (0 = none), lut[0] = 0."""
    things = set(int(c) for c in thing_classes)
    lut = [0] * (len(classes) + 1)
    segments_info = []
    stuff_memory_list = {}
    current_segment_id = 0
    for k, pred_class in enumerate(classes):
        pred_class = int(pred_class)
        mask_area, original_area, intersection = (int(c) for c in counters[k])
        isthing = pred_class in things
        if mask_area > 0 and original_area > 0 and intersection > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            if not isthing:
                if pred_class in stuff_memory_list:
                    lut[k + 1] = stuff_memory_list[pred_class]
                    continue
                stuff_memory_list[pred_class] = current_segment_id + 1
            current_segment_id += 1
            lut[k + 1] = current_segment_id
            segments_info.append({"id": current_segment_id, "isthing": bool(isthing), "category_id": pred_class})
    return lut, segments_info


def _keep_lists(mask_cls, num_classes, object_mask_threshold):
    """(..., Q, K+1) class logits -> kept queries first (ascending), their scores, classes and the count; no sync."""
    scores, labels = F.softmax(mask_cls.float(), dim=-1).max(-1)
    keep = labels.ne(num_classes) & (scores > object_mask_threshold)
    order = torch.sort((~keep).to(torch.uint8), dim=-1, stable=True).indices
    return order, scores.gather(-1, order), labels.gather(-1, order), keep.sum(-1)


def _panoptic_pixels_cpu(full, keep_idx, keep_score, n_keep):
    """winner / inside / counters of the kept queries on full-resolution fp32 logits (Q, H, W), in torch."""
    H, W = full.shape[-2:]
    if n_keep == 0:
        return (torch.full((H, W), -1, dtype=torch.int16), torch.zeros((H, W), dtype=torch.uint8),
                torch.zeros((0, 3), dtype=torch.int32))
    sig = 1.0 / (1.0 + torch.exp(-full[keep_idx[:n_keep]]))
    winner = (keep_score[:n_keep].view(-1, 1, 1) * sig).argmax(0)
    above = sig >= 0.5
    inside = above.gather(0, winner[None])[0]
    counters = torch.stack([torch.bincount(winner.flatten(), minlength=n_keep),
                            above.flatten(1).sum(1),
                            torch.bincount(winner[inside], minlength=n_keep)], dim=1)
    return winner.to(torch.int16), inside.to(torch.uint8), counters.to(torch.int32)


def _apply_lut(winner, inside, lut):
    lut_t = torch.tensor(lut, dtype=torch.int32, device=winner.device)
    return lut_t[winner.long() + 1] * inside.to(torch.int32)


# -------------------------------------------------------------------------------------------------------------------
# kernel launches (batched)
# -------------------------------------------------------------------------------------------------------------------
def _prep(mask_pred, geo):
    if mask_pred.dim() != 4:
        raise ValueError("pred_masks must be (B, Q, h, w)")
    if mask_pred.shape[0] != len(geo):
        raise ValueError("one image size per batch element is required")
    masks = mask_pred.detach().contiguous()
    sizes = torch.tensor(geo, dtype=torch.int32).to(masks.device, non_blocking=True)
    return masks, sizes, max(g[2] for g in geo), max(g[3] for g in geo)


def _semantic_hip(mask_cls, mask_pred, padded_size, geo, labels=False):
    masks, sizes, Ho, Wo = _prep(mask_pred, geo)
    B, Q, h, w = masks.shape
    probs = F.softmax(mask_cls.float(), dim=-1)[..., :-1].transpose(1, 2).contiguous()  # (B, K, Q)
    K = probs.shape[1]
    Hp, Wp = _pair(padded_size)
    if labels:
        out = torch.empty((B, Ho, Wo), dtype=torch.int16, device=masks.device)
        sem_ptr, lab_ptr = None, out.data_ptr()
    else:
        out = torch.empty((B, K, Ho, Wo), dtype=torch.float32, device=masks.device)
        sem_ptr, lab_ptr = out.data_ptr(), None
    _native.call("m2f_infer_semantic", masks.data_ptr(), _native.dtype_code(masks.dtype, "inference masks"),
                 probs.data_ptr(), sizes.data_ptr(), B, Q, K, h, w, Hp, Wp, Ho, Wo, sem_ptr, lab_ptr,
                 _native.stream(masks))
    return [out[b, ..., :g[2], :g[3]] for b, g in enumerate(geo)]


def _panoptic_pass_hip(mask_cls, mask_pred, padded_size, geo, num_classes, object_mask_threshold):
    """-> winner, inside (B, Ho, Wo) on the device and the host copy [counters (Q*3) | classes (Q) | n_keep] (B, .)."""
    masks, sizes, Ho, Wo = _prep(mask_pred, geo)
    B, Q, h, w = masks.shape
    Hp, Wp = _pair(padded_size)
    order, kscore, kclass, n_keep = _keep_lists(mask_cls, num_classes, object_mask_threshold)
    keep_idx = order.to(torch.int32).contiguous()
    kscore = kscore.contiguous()
    n_keep32 = n_keep.to(torch.int32)
    winner = torch.empty((B, Ho, Wo), dtype=torch.int16, device=masks.device)
    inside = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=masks.device)
    counters = torch.empty((B, Q, 3), dtype=torch.int32, device=masks.device)
    _native.call("m2f_infer_panoptic_pass", masks.data_ptr(), _native.dtype_code(masks.dtype, "inference masks"),
                 keep_idx.data_ptr(), kscore.data_ptr(), n_keep32.data_ptr(), sizes.data_ptr(), B, Q, h, w, Hp, Wp, Ho,
                 Wo, winner.data_ptr(), inside.data_ptr(), counters.data_ptr(), _native.stream(masks))
    # the one device-to-host copy of the head: counters, classes and counts of the whole batch
    packed = torch.cat([counters.flatten(1), kclass.to(torch.int32), n_keep32[:, None]], dim=1).cpu()
    return winner, inside, packed


def _panoptic_hip(mask_cls, mask_pred, padded_size, geo, num_classes, thing_classes, object_mask_threshold,
                  overlap_threshold):
    Q = mask_pred.shape[1]
    winner, inside, packed = _panoptic_pass_hip(mask_cls, mask_pred, padded_size, geo, num_classes,
                                                object_mask_threshold)
    results = []
    for b, g in enumerate(geo):
        n = int(packed[b, -1])
        lut, info = merge_segments(packed[b, 3 * Q:3 * Q + n].tolist(), packed[b, :3 * Q].view(Q, 3)[:n].tolist(),
                                   thing_classes, overlap_threshold)
        results.append((_apply_lut(winner[b, :g[2], :g[3]], inside[b, :g[2], :g[3]], lut), info))
    return results


def panoptic_counters(mask_cls, mask_pred, padded_size, image_sizes, output_sizes=None, *, num_classes,
                      object_mask_threshold):
    """Per image the (n_keep, 3) int32 [mask_area, original_area, intersection] rows of the kept queries (in
    ascending query order) that the segment loop consumes; low-resolution (B, Q, h, w) masks, either device."""
    geo = _geometry(padded_size, image_sizes, output_sizes)
    Q = mask_pred.shape[1]
    if _is_hip(mask_pred):
        packed = _panoptic_pass_hip(mask_cls, mask_pred, padded_size, geo, num_classes, object_mask_threshold)[2]
        return [packed[b, :3 * Q].view(Q, 3)[:int(packed[b, -1])].clone() for b in range(len(geo))]
    out = []
    for b, g in enumerate(geo):
        order, kscore, _, n_keep = _keep_lists(mask_cls[b], num_classes, object_mask_threshold)
        full = full_resolution_logits(mask_pred[b], padded_size, g[:2], g[2:])
        out.append(_panoptic_pixels_cpu(full, order, kscore, int(n_keep))[2])
    return out


def _topk(mask_cls, num_classes, topk):
    """scores (.., Q, K+1) -> per image top-k (score, query, class) over the flattened (Q, K) table (:578-584)."""
    scores = F.softmax(mask_cls.float(), dim=-1)[..., :-1]
    s, idx = scores.flatten(-2, -1).topk(topk, sorted=False)
    return s, idx // num_classes, idx % num_classes


def _thing_filter(labels, thing_classes):
    things = torch.tensor(sorted(int(c) for c in thing_classes), dtype=labels.dtype, device=labels.device)
    return torch.isin(labels, things)


def _instance_hip(mask_cls, mask_pred, padded_size, geo, num_classes, topk, thing_classes=None, rle=False):
    """The thing filter of the panoptic setting (:604-611) is applied to the (topk,) lists before the float masks
    are gathered, so only the kept masks are ever expanded.  With ``rle`` the uint8 masks are not expanded at all:
    every live slot's (Ho_b, Wo_b) crop is run-length encoded in place (``csrc/rle.hip``, byte form) and the
    entries index the encoded slots."""
    masks, sizes, Ho, Wo = _prep(mask_pred, geo)
    B, Q, h, w = masks.shape
    Hp, Wp = _pair(padded_size)
    scores, qidx, labels = _topk(mask_cls, num_classes, topk)
    mark = torch.zeros((B, Q), dtype=torch.bool, device=masks.device).scatter_(1, qidx, True)
    order = torch.sort((~mark).to(torch.uint8), dim=1, stable=True).indices   # selected queries first
    rank = torch.sort(order, dim=1).indices                                     # query -> slot
    S = min(Q, topk)
    sel = order[:, :S].to(torch.int32).contiguous()
    n_sel = mark.sum(1).to(torch.int32)
    tiles = (Ho * Wo + _INSTANCE_TILE - 1) // _INSTANCE_TILE
    binary = torch.empty((B, S, Ho, Wo), dtype=torch.uint8, device=masks.device)
    partials = torch.empty((B, S, tiles, 2), dtype=torch.float32, device=masks.device)
    sums = torch.empty((B, S, 2), dtype=torch.float32, device=masks.device)
    _native.call("m2f_infer_instance", masks.data_ptr(), _native.dtype_code(masks.dtype, "inference masks"),
                 sel.data_ptr(), n_sel.data_ptr(), sizes.data_ptr(), B, Q, S, h, w, Hp, Wp, Ho, Wo, tiles,
                 binary.data_ptr(), partials.data_ptr(), sums.data_ptr(), _native.stream(masks))
    results = []
    for b, g in enumerate(geo):
        slot, sc, lab = rank[b].gather(0, qidx[b]), scores[b], labels[b]
        if thing_classes is not None:
            keep = _thing_filter(lab, thing_classes)
            slot, sc, lab = slot[keep], sc[keep], lab[keep]
        sm = sums[b, slot]
        if rle:
            live = torch.arange(S, device=masks.device)
            live = torch.where(live < n_sel[b], live, torch.zeros_like(live)).to(torch.int32)
            enc, slot_h = _encode_device(binary[b, :, :g[2], :g[3]], _BYTES, g[3], plane_index=live, num_masks=S,
                                         extra=slot)
            mask_entry = {"pred_masks_rle": [enc[i] for i in slot_h.tolist()]}
        else:
            mask_entry = {"pred_masks": binary[b, slot, :g[2], :g[3]].float()}
        results.append({**mask_entry,
                        "scores": sc * (sm[:, 0] / (sm[:, 1] + 1e-6)),
                        "pred_classes": lab, "image_size": (g[2], g[3])})
    return results


# -------------------------------------------------------------------------------------------------------------------
# CPU restatement (per image, on full-resolution fp32 logits)
# -------------------------------------------------------------------------------------------------------------------
def _semantic_cpu(mask_cls, full):
    probs = F.softmax(mask_cls.float(), dim=-1)[..., :-1]
    return torch.einsum("qc,qhw->chw", probs, full.sigmoid())


def _panoptic_cpu(mask_cls, full, num_classes, thing_classes, object_mask_threshold, overlap_threshold):
    order, kscore, kclass, n_keep = _keep_lists(mask_cls, num_classes, object_mask_threshold)
    n = int(n_keep)
    winner, inside, counters = _panoptic_pixels_cpu(full, order, kscore, n)
    lut, info = merge_segments(kclass[:n].tolist(), counters.tolist(), thing_classes, overlap_threshold)
    return _apply_lut(winner, inside, lut), info


def _instance_cpu(mask_cls, full, num_classes, topk):
    scores, qidx, labels = _topk(mask_cls, num_classes, topk)
    m = full[qidx]
    binary = (m > 0).float()
    mask_scores = (m.sigmoid().flatten(1) * binary.flatten(1)).sum(1) / (binary.flatten(1).sum(1) + 1e-6)
    return {"pred_masks": binary, "scores": scores * mask_scores, "pred_classes": labels,
            "image_size": tuple(full.shape[-2:])}


def _finish_instances(r, thing_classes):
    """pred_boxes (zeros, :616) and the thing filter of the panoptic setting (:604-611)."""
    if thing_classes is not None:
        keep = _thing_filter(r["pred_classes"], thing_classes)
        r = {k: (v[keep] if torch.is_tensor(v) else v) for k, v in r.items()}
    r["pred_boxes"] = torch.zeros(r["scores"].size(0), 4)
    return r


# -------------------------------------------------------------------------------------------------------------------
# the reference's per-image functions (mask_pred already at full resolution)
# -------------------------------------------------------------------------------------------------------------------
def _is_hip(t):
    return t.device.type == "cuda"


def _identity_geo(mask_pred):
    H, W = mask_pred.shape[-2:]
    return (H, W), [(H, W, H, W)]


def semantic_inference(mask_cls, mask_pred):
    """mask_cls (Q, K+1), mask_pred (Q, H, W) -> (K, H, W) (maskformer_model.py:509-513)."""
    if _is_hip(mask_pred):
        padded, geo = _identity_geo(mask_pred)
        return _semantic_hip(mask_cls[None], mask_pred[None], padded, geo)[0]
    return _semantic_cpu(mask_cls, mask_pred.float())


def panoptic_inference(mask_cls, mask_pred, *, num_classes, thing_classes, object_mask_threshold, overlap_threshold):
    """-> (panoptic_seg (H, W) int32, segments_info) (maskformer_model.py:515-571)."""
    if _is_hip(mask_pred):
        padded, geo = _identity_geo(mask_pred)
        return _panoptic_hip(mask_cls[None], mask_pred[None], padded, geo, num_classes, thing_classes,
                             object_mask_threshold, overlap_threshold)[0]
    return _panoptic_cpu(mask_cls, mask_pred.float(), num_classes, thing_classes, object_mask_threshold,
                         overlap_threshold)


def instance_inference(mask_cls, mask_pred, *, num_classes, test_topk_per_image, thing_classes=None):
    """-> dict(pred_masks, pred_boxes, scores, pred_classes, image_size) (maskformer_model.py:573-624); with
    ``thing_classes`` only those classes are kept (the reference's panoptic_on branch)."""
    if _is_hip(mask_pred):
        padded, geo = _identity_geo(mask_pred)
        return _finish_instances(_instance_hip(mask_cls[None], mask_pred[None], padded, geo, num_classes,
                                               test_topk_per_image, thing_classes)[0], None)
    return _finish_instances(_instance_cpu(mask_cls, mask_pred.float(), num_classes, test_topk_per_image),
                             thing_classes)


class MaskFormerInference(nn.Module):
    """The eval branch of MaskFormer.forward on the decoder's low-resolution outputs."""

    def __init__(self, *, num_classes, thing_classes=(), semantic_on=True, instance_on=False, panoptic_on=False,
                 object_mask_threshold=0.8, overlap_threshold=0.8, sem_seg_postprocess_before_inference=False,
                 test_topk_per_image=100):
        super().__init__()
        if not 0 < num_classes <= _MAX_K:
            raise ValueError(f"num_classes {num_classes} outside [1, {_MAX_K}]")
        self.num_classes = int(num_classes)
        self.thing_classes = tuple(sorted(int(c) for c in thing_classes))
        self.semantic_on, self.instance_on, self.panoptic_on = bool(semantic_on), bool(instance_on), bool(panoptic_on)
        self.object_mask_threshold = float(object_mask_threshold)
        self.overlap_threshold = float(overlap_threshold)
        # the reference's or-rule (maskformer_model.py:237-241)
        self.sem_seg_postprocess_before_inference = bool(sem_seg_postprocess_before_inference or panoptic_on
                                                         or instance_on)
        self.test_topk_per_image = int(test_topk_per_image)

    @classmethod
    def from_config(cls, cfg, metadata):
        t = cfg.MODEL.MASK_FORMER.TEST
        things = getattr(metadata, "thing_dataset_id_to_contiguous_id", None) or {}
        return cls(num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, thing_classes=things.values(),
                   semantic_on=t.SEMANTIC_ON, instance_on=t.INSTANCE_ON, panoptic_on=t.PANOPTIC_ON,
                   object_mask_threshold=t.OBJECT_MASK_THRESHOLD, overlap_threshold=t.OVERLAP_THRESHOLD,
                   sem_seg_postprocess_before_inference=t.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE,
                   test_topk_per_image=cfg.TEST.DETECTIONS_PER_IMAGE)

    def forward(self, outputs, padded_size, image_sizes, output_sizes=None, semantic_labels=False,
                instance_rle=False):
        """outputs: {"pred_logits": (B, Q, K+1), "pred_masks": (B, Q, h, w)}; padded_size: (Hp, Wp) of the padded
        batch; image_sizes: (Hc, Wc) per image; output_sizes: (height, width) per image (default: the image size).
        Returns one dict per image keyed as the reference's processed_results.  With ``semantic_labels`` the
        semantic head returns ``"sem_seg_labels"`` (int16 argmax map) instead of the (K, H, W) scores.  With
        ``instance_rle`` each image's ``"instances"`` holds ``pred_masks_rle``, a list of COCO RLE dicts
        (``bm2f_amd.rle``) at that image's output size, in place of the float ``pred_masks``."""
        mask_cls, mask_pred = outputs["pred_logits"], outputs["pred_masks"]
        B, Q = mask_pred.shape[:2]
        if mask_cls.shape[-1] != self.num_classes + 1:
            raise ValueError(f"pred_logits has {mask_cls.shape[-1]} columns, expected num_classes + 1")
        if Q > _MAX_Q:
            raise ValueError(f"{Q} queries > {_MAX_Q}")
        geo = _geometry(padded_size, image_sizes, output_sizes)
        if len(geo) != B:
            raise ValueError("one image size per batch element is required")
        before = self.sem_seg_postprocess_before_inference
        # without postprocessing before inference the semantic scores are computed on the crop and resized after
        sem_geo = geo if before else [(g[0], g[1], g[0], g[1]) for g in geo]
        if semantic_labels and sem_geo != geo:
            raise ValueError("semantic_labels needs sem_seg_postprocess_before_inference or output size == image size")
        results = [{} for _ in range(B)]
        hip = _is_hip(mask_pred)
        things = self.thing_classes
        if not hip:
            full = [full_resolution_logits(mask_pred[b], padded_size, g[:2], g[2:]) for b, g in enumerate(geo)]
            sem_full = full if before else [full_resolution_logits(mask_pred[b], padded_size, g[:2])
                                            for b, g in enumerate(geo)]
        if self.semantic_on:
            if hip:
                sem = _semantic_hip(mask_cls, mask_pred, padded_size, sem_geo, labels=semantic_labels)
            else:
                sem = [_semantic_cpu(mask_cls[b], sem_full[b]) for b in range(B)]
                if semantic_labels:
                    sem = [s.argmax(0).to(torch.int16) for s in sem]
            for b, g in enumerate(geo):
                r = sem[b]
                if not before and (g[2], g[3]) != (g[0], g[1]):
                    r = F.interpolate(r[None], size=(g[2], g[3]), mode="bilinear", align_corners=False)[0]
                results[b]["sem_seg_labels" if semantic_labels else "sem_seg"] = r
        if self.panoptic_on:
            if hip:
                pan = _panoptic_hip(mask_cls, mask_pred, padded_size, geo, self.num_classes, things,
                                    self.object_mask_threshold, self.overlap_threshold)
            else:
                pan = [_panoptic_cpu(mask_cls[b], full[b], self.num_classes, things, self.object_mask_threshold,
                                     self.overlap_threshold) for b in range(B)]
            for b in range(B):
                results[b]["panoptic_seg"] = pan[b]
        if self.instance_on:
            ins_things = things if self.panoptic_on else None
            if hip:
                ins = _instance_hip(mask_cls, mask_pred, padded_size, geo, self.num_classes, self.test_topk_per_image,
                                    ins_things, rle=instance_rle)
                ins_things = None   # already applied
            else:
                ins = [_instance_cpu(mask_cls[b], full[b], self.num_classes, self.test_topk_per_image)
                       for b in range(B)]
            for b in range(B):
                r = _finish_instances(ins[b], ins_things)
                if instance_rle and not hip:
                    r["pred_masks_rle"] = rle_encode(r.pop("pred_masks") > 0)
                results[b]["instances"] = r
        return results
