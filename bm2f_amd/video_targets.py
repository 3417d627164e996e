"""Clip target preparation: the reference's ``VideoMaskFormer.prepare_weaksup_targets``
(mask2former_video/video_maskformer_model.py:395-620) and ``prepare_targets`` (:622-649) without their host loops.

What the reference does per frame or per (instance, frame) is done here for the whole batch of clips at once:

* Lab conversion and colour similarity: one ``m2f_weaksup_lab`` and one ``m2f_color_similarity`` launch over all B*T
  frames (the reference copies every frame to the host for ``rgb2lab``);
* box rasters, projection bounds and the stride-4 boxes used for mining: analytic, from the boxes' integers, for all
  (instance, frame) at once (the reference loops with ``argmax`` / ``flip`` over full-resolution rasters);
* DINO features: ``m2f_feat_resize_pad`` (``csrc/video_inference.hip``) reads the unpadded features and writes the
  stride-4 map; the zero-padded full-resolution copy (T, D, Hp, Wp) the reference interpolates from is never built;
* temporal pairs: one :func:`bm2f_amd.weaksup.temporal_pairs` call per clip (one mining launch) where the reference
  calls ``get_instance_temporal_pairs`` per (instance, frame pair).

On CPU tensors the same definitions run in plain torch, so the host logic is testable without a GPU; on a HIP tensor a
kernel error raises, there is no fall-back.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _native
from . import weaksup as ws
from .inference import _pair


def _frames(clip, num_frames):
    frames = clip["instances"] if isinstance(clip, dict) and "instances" in clip else clip
    if len(frames) != num_frames:
        raise ValueError(f"a clip has {len(frames)} frames, expected num_frames = {num_frames}")
    return frames


def _fields(frame):
    """(boxes (G, 4), labels, ids, masks (G, H, W), image_size) of a detectron2 Instances or a dict."""
    if isinstance(frame, dict):
        return frame["boxes"], frame["labels"], frame["ids"], frame["masks"], frame["image_size"]
    masks = frame.gt_masks
    boxes = frame.gt_boxes
    return (getattr(boxes, "tensor", boxes), frame.gt_classes, frame.gt_ids, getattr(masks, "tensor", masks),
            frame.image_size)


def _ids_labels(frames, device):
    """ids (G, T) on the host and the device, labels of the last frame (:599-603)."""
    ids = torch.cat([_fields(f)[2].reshape(-1, 1) for f in frames], dim=1)
    keep = (ids.cpu() != -1).any(dim=-1).nonzero().flatten()
    return ids.to(device), _fields(frames[-1])[1].to(device), keep.to(device)


# -------------------------------------------------------------------------------------------------------------------
# DINO feature resize
# -------------------------------------------------------------------------------------------------------------------
def feat_resize_pad(feats: torch.Tensor, padded_size, out_size) -> torch.Tensor:
    """(..., H', W') features (fp32 / fp16 / bf16) -> (..., oh, ow) fp32: bilinear ``F.interpolate``
    (align_corners=False) of the features zero-padded bottom/right to ``padded_size`` (:508-517).  On a HIP tensor
    the padded copy is never built (``m2f_feat_resize_pad``).  The tap weights are exact (integer arithmetic on the
    device, fp64 on the CPU) and the result is rounded to fp32: at an integer ratio such as the stride-4 resize it
    is the reference's fp32 result bit for bit; at other ratios it is closer to the exact interpolation than fp32
    ``F.interpolate``, whose coordinate rounding alone costs about 1e-5 of the feature range."""
    Hp, Wp = _pair(padded_size)
    oh, ow = _pair(out_size)
    Hs, Ws = feats.shape[-2:]
    if not (0 < Hs <= Hp and 0 < Ws <= Wp and oh > 0 and ow > 0):
        raise ValueError(f"features {(Hs, Ws)} do not fit the padded size {(Hp, Wp)}")
    lead = tuple(feats.shape[:-2])
    if feats.is_cuda:
        x = feats.detach().contiguous()
        out = torch.empty(lead + (oh, ow), dtype=torch.float32, device=x.device)
        planes = x.numel() // (Hs * Ws)
        if planes:
            _native.call("m2f_feat_resize_pad", x.data_ptr(), _native.dtype_code(x.dtype, "feat_resize_pad"), planes,
                         Hs, Ws, Hp, Wp, oh, ow, out.data_ptr(), _native.stream(x))
        return out
    x = F.pad(feats.double().reshape(1, -1, Hs, Ws), (0, Wp - Ws, 0, Hp - Hs))
    return F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False).float().reshape(lead + (oh, ow))


def _clip_feats(feats, num_frames, padded_size, out_size):
    """One clip's features -- a (T, D, H', W') tensor or T tensors (D, H', W') / (1, D, H', W') -- at stride 4; a
    list is resized frame by frame, so the frames are never concatenated at full resolution."""
    if torch.is_tensor(feats):
        if feats.dim() != 4 or feats.shape[0] != num_frames:
            raise ValueError("org_dino_feats of a clip must be (T, D, H', W')")
        return feat_resize_pad(feats, padded_size, out_size)
    if len(feats) != num_frames:
        raise ValueError("org_dino_feats needs one entry per frame")
    return torch.stack([feat_resize_pad(f[0] if f.dim() == 4 else f, padded_size, out_size) for f in feats])


# -------------------------------------------------------------------------------------------------------------------
# Lab and colour similarity on CPU tensors (the kernels' definitions in torch)
# -------------------------------------------------------------------------------------------------------------------
def _images_lab_torch(images, stride):
    """avg_pool, .byte(), skimage.color.rgb2lab in float64 (:421-424, :463-464) -> fp32 (N, 3, h, w)."""
    a = F.avg_pool2d(images.float(), kernel_size=stride, stride=stride).clamp(0, 255).to(torch.uint8).double() / 255.0
    a = torch.where(a > 0.04045, ((a + 0.055) / 1.055) ** 2.4, a / 12.92)
    r, g, b = a[:, 0], a[:, 1], a[:, 2]
    xyz = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047, 0.212671 * r + 0.715160 * g + 0.072169 * b, \
        (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883
    fx, fy, fz = (torch.where(t > 0.008856, t ** (1.0 / 3.0), 7.787 * t + 16.0 / 116.0) for t in xyz)
    return torch.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], 1).float()


def _neighbours(x, d):
    """(N, C, H, W) -> (N, C, 8, H, W): the 3x3 dilated taps minus the centre, zero outside (unfold_wo_center)."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (d, d, d, d))
    return torch.stack([xp[..., ky * d:ky * d + H, kx * d:kx * d + W]
                        for ky in range(3) for kx in range(3) if (ky, kx) != (1, 1)], 2)


def _color_similarity_torch(lab, mask, d):
    """get_images_color_similarity (utils/weaksup_utils.py:37-61): lab (N, 3, h, w), mask (N, h, w) -> (N, 8, h, w)."""
    diff = lab[:, :, None] - _neighbours(lab, d)
    return torch.exp(-torch.norm(diff, dim=1) * 0.5) * _neighbours(mask[:, None].float(), d)[:, 0]


# -------------------------------------------------------------------------------------------------------------------
# targets
# -------------------------------------------------------------------------------------------------------------------
def _strided_masks(frames, G, T, Hp, Wp, start, stride, device):
    """gt masks zero-padded to (Hp, Wp) and sampled at the stride grid (:459, :494), without the padded copy."""
    out = torch.zeros((G, T, Hp // stride, Wp // stride), dtype=torch.float32, device=device)
    for t, f in enumerate(frames):
        m, (ih, iw) = _fields(f)[3], _fields(f)[4]
        sub = m.to(device)[:, :ih, :iw][:, start::stride, start::stride]
        out[:, t, :sub.shape[1], :sub.shape[2]] = sub
    return out


def calculate_matching_pos(pairs: ws.MinedPairs, masks: torch.Tensor) -> torch.Tensor:
    """The reference's debug counter (:697-701) on packed pairs: how many pairs join pixels with the same mask
    label; masks (G, T, h, w)."""
    if pairs.g.numel() == 0:
        return torch.zeros((), dtype=torch.float32, device=masks.device)
    G, T, h, w = masks.shape
    flat = masks.reshape(G, -1)
    g, t = pairs.g.long(), pairs.t.long()
    a = flat[g, t * (h * w) + pairs.p0.long()]
    b = flat[g, (t + 1) * (h * w) + pairs.p1.long()]
    return ((a - b) == 0).float().sum()


def prepare_video_weaksup_targets(targets, org_images, org_dino_feats=None, *, num_frames, size_divisibility=32,
                                  mask_out_stride=4, pairwise_size=3, pairwise_dilation=2, temporal_k=1):
    """``VideoMaskFormer.prepare_weaksup_targets`` (video_maskformer_model.py:395-620).

    targets: per clip a list of T frames (or a dict with ``"instances"``), each a detectron2 ``Instances``
    (``gt_boxes``, ``gt_classes``, ``gt_ids``, ``gt_masks``, ``image_size``) or a dict with ``boxes`` (G, 4) x0, y0,
    x1, y1, ``labels``, ``ids``, ``masks`` (G, H, W) and ``image_size``; org_images: the B*T frames (3, H, W), 0..255;
    org_dino_feats: per clip a (T, D, H', W') tensor or T tensors (D, H', W') / (1, D, H', W'), or None (no mining).

    Returns the reference's per-clip dicts: ``labels``, ``ids``, ``box_masks``, ``masks`` (G, T, h, w), the four
    bounds, ``color_similarities`` (G, T, 8, h, w) -- a stride-0 ``expand`` of the frames' one map over the instances,
    where the reference materialises G copies -- ``temporal_pairs``, ``total_temp_pair`` and ``pos_temp_pair``.

    Differences: ``temporal_pairs`` is a :class:`bm2f_amd.weaksup.MinedPairs` of the *returned* targets (the
    instances of ``valid_idx``, one entry per target, as the criterion requires); the reference leaves its list over
    all instances unfiltered (:615), so it is longer than its other entries whenever an instance is absent from every
    frame.  The two counters are taken over the same valid instances (an instance without a box in any frame mines
    nothing, so they agree with the reference's).  A clip without instances yields empty tensors.  Boxes are taken
    as non-negative pixel coordinates (as detectron2 clips them)."""
    if pairwise_size != 3:
        raise ValueError("only pairwise_size 3 is implemented")
    B, T = len(targets), int(num_frames)
    if len(org_images) != B * T:
        raise ValueError("org_images needs B * num_frames frames")
    dev = org_images[0].device
    stride = int(mask_out_stride)
    start = stride // 2
    images = ws._pad_stack([x.float() for x in org_images], size_divisibility, 0.0)            # (B*T, 3, Hp, Wp)
    image_masks = ws._pad_stack([torch.ones(x.shape[-2:], dtype=torch.float32, device=dev) for x in org_images],
                                size_divisibility, 0.0)
    Hp, Wp = images.shape[-2:]
    if Hp % stride or Wp % stride:
        raise ValueError("padded image size must be a multiple of mask_out_stride")
    h, w = Hp // stride, Wp // stride
    ds_masks = image_masks[:, start::stride, start::stride]
    if images.is_cuda:
        sim = ws.color_similarity(ws.images_lab(images, stride), ds_masks, pairwise_dilation)
    else:
        sim = _color_similarity_torch(_images_lab_torch(images, stride), ds_masks, pairwise_dilation)
    sim = sim.view(B, T, 8, h, w)
    ys = start + stride * torch.arange(h, device=dev)
    xs = start + stride * torch.arange(w, device=dev)
    out = []
    for b, clip in enumerate(targets):
        frames = _frames(clip, T)
        boxes = torch.stack([_fields(f)[0].to(dev).float().reshape(-1, 4) for f in frames], dim=1)   # (G, T, 4)
        G = boxes.shape[0]
        ids, labels, keep = _ids_labels(frames, dev)
        # python int(): truncation toward zero; slices [y0, y1 + 1) clipped to the padded frame (:475-477)
        ib = boxes.trunc().long()
        x0, y0 = ib[..., 0], ib[..., 1]
        x1 = ib[..., 2].clamp(max=Wp - 1)
        y1 = ib[..., 3].clamp(max=Hp - 1)
        in_y = (ys >= y0[..., None]) & (ys <= y1[..., None])                                   # (G, T, h)
        in_x = (xs >= x0[..., None]) & (xs <= x1[..., None])                                   # (G, T, w)
        box_masks = (in_y[..., :, None] & in_x[..., None, :]).float()
        # argmax of a box row = its first column (0 for an empty row); W - argmax(flipped) = last + 1 (or W).  An
        # absent instance's zero box is the single pixel (0, 0), which no strided row or column meets
        row_on = in_y & (x1 >= x0)[..., None]
        col_on = in_x & (y1 >= y0)[..., None]
        left = torch.where(row_on, x0[..., None].float(), 0.0) / stride
        right = torch.where(row_on, (x1 + 1)[..., None].float(), float(Wp)) / stride
        top = torch.where(col_on, y0[..., None].float(), 0.0) / stride
        bottom = torch.where(col_on, (y1 + 1)[..., None].float(), float(Hp)) / stride
        masks = _strided_masks(frames, G, T, Hp, Wp, start, stride, dev)
        t = {"labels": labels[keep], "ids": ids[keep], "box_masks": box_masks[keep], "masks": masks[keep],
             "left_bounds": left[keep], "right_bounds": right[keep], "top_bounds": top[keep],
             "bottom_bounds": bottom[keep],
             "color_similarities": sim[b][None].expand(keep.numel(), T, 8, h, w),
             "temporal_pairs": None, "total_temp_pair": None, "pos_temp_pair": None}
        if org_dino_feats is not None:
            # BitMasks.get_bounding_boxes of the strided raster (:519-521): the first and last grid index inside
            # the box per axis, half-open; zeros for an empty raster
            div = lambda a: torch.div(a, stride, rounding_mode="floor")  # noqa: E731
            yi0, yi1 = (-div(start - y0)).clamp(min=0), div(y1 - start).clamp(max=h - 1)
            xi0, xi1 = (-div(start - x0)).clamp(min=0), div(x1 - start).clamp(max=w - 1)
            on = ((yi1 >= yi0) & (xi1 >= xi0))[..., None]
            box4 = torch.where(on, torch.stack([xi0, yi0, xi1 + 1, yi1 + 1], -1), 0)
            feats = _clip_feats(org_dino_feats[b], T, (Hp, Wp), (h, w))
            pairs = ws.temporal_pairs(feats, box4[keep], k=temporal_k)
            t["temporal_pairs"] = pairs
            t["total_temp_pair"] = torch.tensor(float(pairs.g.numel()), dtype=torch.float32, device=dev)
            t["pos_temp_pair"] = calculate_matching_pos(pairs, t["masks"])
        out.append(t)
    return out


def prepare_video_targets(targets, padded_size, num_frames):
    """``VideoMaskFormer.prepare_targets`` (video_maskformer_model.py:622-649): per clip ``labels``, ``ids`` (G, T)
    and the full-resolution ``masks`` (G, T, Hp, Wp) fp32 of the instances present in some frame."""
    Hp, Wp = _pair(padded_size)
    out = []
    for clip in targets:
        frames = _frames(clip, int(num_frames))
        dev = _fields(frames[0])[3].device
        ids, labels, keep = _ids_labels(frames, dev)
        masks = torch.zeros((ids.shape[0], len(frames), Hp, Wp), dtype=torch.bool, device=dev)
        for t, f in enumerate(frames):
            m, (ih, iw) = _fields(f)[3], _fields(f)[4]
            masks[:, t, :ih, :iw] = m.to(dev)
        out.append({"labels": labels[keep], "ids": ids[keep], "masks": masks[keep].float()})
    return out
