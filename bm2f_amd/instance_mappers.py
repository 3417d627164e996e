"""Instance and video-instance training mappers on the device: per-instance masks and tight boxes under the views.

The reference's headline configs train from per-instance annotations.  Its mappers turn each annotation into a
transformed mask and a tight box:

  :class:`InstanceTrainMapper`        ``MaskFormerInstanceDatasetMapper`` (the semantic mapper's augmentations)
  :class:`COCOInstanceLSJMapper`      ``COCOInstanceNewBaselineDatasetMapper`` (flip, large-scale jitter, fixed crop)
  :class:`VideoInstanceTrainMapper`   ``YTVISDatasetMapper``, training branch (:func:`sample_clip_frames` is its frame
                                      selection)

All take samples already uploaded and a ``numpy.random.Generator``; ``views=`` replays a draw.  The images come from
one ``image_views`` call, as in :mod:`bm2f_amd.train_mappers`.  An annotation is a dict with ``"segmentation"``,
``"category_id"`` (the contiguous class index), optionally ``"iscrowd"`` (such annotations are dropped) and, for video,
``"id"``; ``"keypoints"`` is ignored.  A segmentation is a COCO polygon list, an RLE dict (compressed or uncompressed)
or an (H, W) uint8 / bool array or tensor.

RLE and array annotations are decoded at source size (``rle_to_bits_ragged`` / ``pack_mask_bits``) and go through
:func:`~bm2f_amd.instance_views.instance_views`: ``transform_instance_annotations`` on a decoded uint8 mask (PIL
``NEAREST`` resize, crop, flip, zero pad), then ``BitMasks.get_bounding_boxes``.

Polygon annotations: the host applies the view's affine map to the vertices in the mapper's transform order
(:func:`transform_polygons`: flip ``x -> W - x``, resize ``x -> x rw / W``, ``y -> y rh / H``, crop ``- (cx0, cy0)``,
flip of the crop ``x -> cw - x``), the planes are rasterised once at the output size with ``polygons_to_bits_ragged``
(which clips to the plane) and the boxes and areas come from ``bit_boxes_ragged``.  **Stated deviation**: detectron2's
``CropTransform.apply_polygons`` clips polygons with shapely before rasterising, and ``PolygonMasks.get_bounding_boxes``
is the vertex min / max of the clipped polygons; here the unclipped polygon is rasterised on the canvas and the box is
the tight box of those pixels.  shapely and detectron2 are not installed where this was written and were never run
against it.  Polygon vertices are taken to lie inside the source image (nothing is cut at the image's edge inside a
crop that reaches past it).

Not claimed: the draws follow the distributions and the order of the reference's augmentation lists, not the bit
stream of detectron2's ``random``.  Out of scope: ``CocoClipDatasetMapper``, rotation, the source-space
``T.RandomCrop`` of the video mappers, vertical flips and reading files.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from .image_views import View, image_views, lsj_view
from .instance_views import bit_boxes_ragged, instance_views
from .mask_iou import rle_to_bits_ragged
from .polygon import is_polygon, polygons_to_bits_ragged
from .train_mappers import SemanticTrainMapper, video_clip_views
from .video_inference import pack_mask_bits


# ------------------------------------------------------------------------------------------------ geometry
def _geometry(view, hw):
    """(rh, rw, cy0, cx0, ch, cw, Hc, Wc) of a view of an (H, W) source."""
    rh, rw = (int(s) for s in view.size)
    crop = (0, 0, rh, rw) if view.crop is None else tuple(int(s) for s in view.crop)
    canvas = crop[2:] if view.canvas is None else tuple(int(s) for s in view.canvas)
    return (rh, rw) + crop + canvas


def transform_polygons(polys, view, hw):
    """The view's affine map on a polygon segmentation (a list of flat ``[x0, y0, x1, y1, ...]`` lists) of an (H, W)
    image, in float64: -> a list of flat arrays in canvas coordinates.  Nothing is clipped."""
    H, W = hw
    rh, rw, cy0, cx0, ch, cw, _, _ = _geometry(view, hw)
    out = []
    for p in polys:
        a = np.array(p, dtype=np.float64).reshape(-1, 2)
        x, y = a[:, 0], a[:, 1]
        if view.flip_in:
            x = W - x
        x, y = x * (rw / W), y * (rh / H)
        x, y = x - cx0, y - cy0
        if view.flip_out:
            x = cw - x
        out.append(np.stack((x, y), axis=1).reshape(-1))
    return out


def _plane_size(view, hw):
    """The part of the canvas a polygon can show in: the crop window cut by the canvas."""
    _, _, _, _, ch, cw, Hc, Wc = _geometry(view, hw)
    return min(ch, Hc), min(cw, Wc)


def padding_masks(views, shapes, padded, device):
    """(V, Hp, Wp) bool, True where a view does not show its image (canvas fill and batch pad), from the geometry
    alone: one small upload of the per-axis flags and an outer product on the device."""
    Hp, Wp = padded
    rows, cols = np.zeros((len(views), Hp), dtype=bool), np.zeros((len(views), Wp), dtype=bool)
    for i, v in enumerate(views):
        rh, rw, cy0, cx0, ch, cw, Hc, Wc = _geometry(v, shapes[v.source])
        y, x = np.arange(Hp), np.arange(Wp)
        rx = cx0 + (cw - 1 - x if v.flip_out else x)
        rows[i] = (y < min(ch, Hc)) & (cy0 + y >= 0) & (cy0 + y < rh)
        cols[i] = (x < min(cw, Wc)) & (rx >= 0) & (rx < rw)
    flags = torch.from_numpy(np.concatenate((rows, cols), axis=1)).to(device)
    return ~(flags[:, :Hp, None] & flags[:, None, Hp:])


# ------------------------------------------------------------------------------------------------ masks of a batch
def _kept(annotations):
    return [a for a in annotations if not int(a.get("iscrowd", 0))]


def view_masks(segs, view_of_seg, views, shapes, device, out="uint8"):
    """The segmentations ``segs`` (``segs[k]`` under ``views[view_of_seg[k]]``, whose source is ``shapes[v.source]``)
    -> ``(masks, boxes (K, 4) float32, areas (K,) int32)`` on ``device`` in the order of ``segs``: ``masks`` (K, Hm,
    Wm) uint8 or (K, Hm, ceil(Wm / 32)) int32 bit planes with (Hm, Wm) the largest canvas; a view's masks are zero
    beyond its own canvas.  Decoded annotations take the ``instance_views`` route, polygons the ``bit_boxes_ragged``
    route; a batch of one kind is one route's output as it is."""
    device = torch.device(device)
    K = len(segs)
    canv = [_geometry(v, shapes[v.source])[6:] for v in views]
    Hm, Wm = max(c[0] for c in canv), max(c[1] for c in canv)
    width = Wm if out == "uint8" else (Wm + 31) // 32
    if K == 0:
        return (torch.zeros((0, Hm, width), dtype=torch.uint8 if out == "uint8" else torch.int32, device=device),
                torch.zeros((0, 4), dtype=torch.float32, device=device),
                torch.zeros(0, dtype=torch.int32, device=device))
    poly = [k for k in range(K) if is_polygon(segs[k])]
    dec = [k for k in range(K) if not is_polygon(segs[k])]
    parts = []
    if dec:
        rles = [segs[k] if isinstance(segs[k], dict) else None for k in dec]
        src = [tuple(shapes[views[view_of_seg[k]].source]) for k in dec]
        for k, r, s in zip(dec, rles, src):
            own = tuple(int(v) for v in (r["size"] if r is not None else segs[k].shape))
            if own != tuple(int(v) for v in s):
                raise ValueError(f"segmentation {k} is {own}, its image is {s}")
        words, offsets, sizes = rle_to_bits_ragged(rles, device, src)
        arrays, at = [], words.numel()
        for j, k in enumerate(dec):
            if rles[j] is None:                               # an array: packed on the device, appended to the buffer
                a = pack_mask_bits(torch.as_tensor(segs[k]).to(device) != 0).reshape(-1)
                arrays.append(a)
                offsets[j] = at
                at += a.numel()
        if arrays:
            words = torch.cat([words] + arrays)
        vom = np.array([view_of_seg[k] for k in dec], dtype=np.int64)
        parts.append((dec, instance_views(words, offsets, sizes, vom, views, out=out)[:3]))
    if poly:
        moved = [transform_polygons(segs[k], views[view_of_seg[k]], shapes[views[view_of_seg[k]].source])
                 for k in poly]
        sizes = [_plane_size(views[view_of_seg[k]], shapes[views[view_of_seg[k]].source]) for k in poly]
        words, offsets, sizes = polygons_to_bits_ragged(moved, sizes, device)
        parts.append((poly, bit_boxes_ragged(words, offsets, sizes, out=out)))
    if len(parts) == 1:
        masks, boxes, areas = parts[0][1]
        if masks.shape[1:] != (Hm, width):                    # polygon planes smaller than the largest canvas
            masks = F.pad(masks, (0, width - masks.shape[2], 0, Hm - masks.shape[1]))
        return masks, boxes, areas
    order = torch.as_tensor(np.argsort(np.array(parts[0][0] + parts[1][0]), kind="stable"), device=device)
    masks = torch.cat([F.pad(m, (0, width - m.shape[2], 0, Hm - m.shape[1])) for _, (m, _, _) in parts])
    return (masks[order], torch.cat([p[1][1] for p in parts])[order], torch.cat([p[1][2] for p in parts])[order])


def _cut(masks, canvas, out):
    """A view's masks cut to its own canvas: a slice of the batch tensor, no copy."""
    h, w = canvas
    return masks[:, :h, :w] if out == "uint8" else masks[:, :h, :(w + 31) // 32]


def _per_image(annotations, views, shapes, device, out):
    """-> per image ``{"labels", "masks", "boxes"}`` for annotation lists already filtered."""
    segs = [a["segmentation"] for anns in annotations for a in anns]
    vos = [i for i, anns in enumerate(annotations) for _ in anns]
    masks, boxes, _ = view_masks(segs, vos, views, shapes, device, out)
    result, at = [], 0
    for i, anns in enumerate(annotations):
        n = len(anns)
        labels = torch.tensor([int(a["category_id"]) for a in anns], dtype=torch.int64)
        canvas = _geometry(views[i], shapes[views[i].source])[6:]
        result.append({"labels": labels.to(device), "masks": _cut(masks[at:at + n], canvas, out),
                       "boxes": boxes[at:at + n]})
        at += n
    return result


# ------------------------------------------------------------------------------------------------ image mappers
class InstanceTrainMapper(SemanticTrainMapper):
    """``MaskFormerInstanceDatasetMapper`` plus the model's normalisation: the config values and the views of
    :class:`~bm2f_amd.train_mappers.SemanticTrainMapper` (``ignore_label`` is not used) on ``(image uint8 (H, W, 3),
    annotations)`` samples.  Returns ``"images"``, ``"image_sizes"``, ``"views"`` and ``"instances"``: per image
    ``{"labels", "masks", "boxes"}`` on the image's ``SIZE_DIVISIBILITY`` canvas, ``masks`` (G, Hc, Wc) uint8 (or bit
    planes with ``mask_format="bits"``).  An instance the crop left empty is kept with a zero box, as the reference
    keeps it; ``prepare_weaksup_targets`` and ``mask_criterion.SetCriterion`` take the dicts as they are."""

    def __init__(self, *, mask_format="uint8", ignore_label=255, **kw):
        super().__init__(ignore_label=ignore_label, **kw)
        self.mask_format = mask_format

    def __call__(self, samples, rng=None, views=None):
        rng = np.random.default_rng() if rng is None else rng
        images = [s[0] for s in samples]
        shapes = [tuple(im.shape[:2]) for im in images]
        if views is None:
            views = self.draw_views(shapes, rng)
        batch, sizes = image_views(images, views, pixel_mean=self.pixel_mean, pixel_std=self.pixel_std,
                                   out_dtype=self.out_dtype, size_divisibility=self.batch_divisibility)
        instances = _per_image([_kept(s[1]) for s in samples], views, shapes, batch.device, self.mask_format)
        return {"images": batch, "image_sizes": sizes, "views": views, "instances": instances}


class COCOInstanceLSJMapper:
    """``COCOInstanceNewBaselineDatasetMapper`` plus the model's normalisation.  Config values: ``image_size``,
    ``min_scale``, ``max_scale`` (``INPUT.IMAGE_SIZE`` / ``MIN_SCALE`` / ``MAX_SCALE``), ``random_flip``
    ("horizontal" or "none"), ``pixel_mean`` / ``pixel_std``; ``batch_divisibility`` is the model's rounding.

    Per image the draws are, in the order of the reference's list (``RandomFlip``, ``ResizeScale``, ``FixedSizeCrop``):
    the flip coin, ``scale ~ U[min_scale, max_scale]`` and one ``offset_frac ~ U[0, 1)``; the view is
    :func:`~bm2f_amd.image_views.lsj_view`.  Then ``filter_empty_instances``: a row is dropped when ``x1 - x0 <= 1e-5``
    or ``y1 - y0 <= 1e-5`` (this reads the boxes: one device-to-host copy per batch).  Returns ``"images"``,
    ``"image_sizes"``, ``"views"``, ``"instances"`` as :class:`InstanceTrainMapper` and ``"padding_mask"`` (B, Hp, Wp)
    bool, True outside the image, computed from the view geometry."""

    def __init__(self, *, image_size, min_scale, max_scale, pixel_mean, pixel_std, random_flip="horizontal",
                 batch_divisibility=0, out_dtype=torch.float32, mask_format="uint8"):
        if random_flip not in ("horizontal", "none"):
            raise ValueError(f"random_flip {random_flip!r} is not horizontal or none (vertical is out of scope)")
        self.image_size = int(image_size)
        self.min_scale, self.max_scale = float(min_scale), float(max_scale)
        self.random_flip = random_flip
        self.pixel_mean, self.pixel_std = pixel_mean, pixel_std
        self.batch_divisibility = int(batch_divisibility)
        self.out_dtype = out_dtype
        self.mask_format = mask_format

    def draw_views(self, shapes, rng):
        views = []
        for i, (h, w) in enumerate(shapes):
            flip = bool(rng.random() < 0.5) if self.random_flip == "horizontal" else False
            scale = float(rng.uniform(self.min_scale, self.max_scale))
            views.append(lsj_view(h, w, self.image_size, scale, float(rng.random()), flip, source=i))
        return views

    def __call__(self, samples, rng=None, views=None):
        rng = np.random.default_rng() if rng is None else rng
        images = [s[0] for s in samples]
        shapes = [tuple(im.shape[:2]) for im in images]
        if views is None:
            views = self.draw_views(shapes, rng)
        batch, sizes = image_views(images, views, pixel_mean=self.pixel_mean, pixel_std=self.pixel_std,
                                   out_dtype=self.out_dtype, size_divisibility=self.batch_divisibility)
        instances = _per_image([_kept(s[1]) for s in samples], views, shapes, batch.device, self.mask_format)
        boxes = torch.cat([t["boxes"] for t in instances])
        keep = ((boxes[:, 2] - boxes[:, 0] > 1e-5) & (boxes[:, 3] - boxes[:, 1] > 1e-5)).cpu()      # the one copy
        at = 0
        for t in instances:
            k = keep[at:at + t["labels"].numel()]
            at += k.numel()
            if not bool(k.all()):
                idx = k.nonzero().flatten().to(batch.device)
                t.update({key: t[key][idx] for key in ("labels", "masks", "boxes")})
        pad = padding_masks(views, shapes, tuple(batch.shape[-2:]), batch.device)
        return {"images": batch, "image_sizes": sizes, "views": views, "instances": instances, "padding_mask": pad}


# ------------------------------------------------------------------------------------------------ video
def sample_clip_frames(video_length, rng, sampling_frame_num=2):
    """``YTVISDatasetMapper``'s training frame selection: the interval is 4 / 10 / 15 / 20 / 36 for a length ``<= 10`` /
    ``<= 20`` / ``<= 30`` / ``<= 40`` / longer, ``ref`` uniform in ``[0, length - interval)`` and the target ``ref +
    interval``: -> ``[ref, ref + interval]``.  A video not longer than its interval raises ValueError (the reference's
    ``randrange`` raises there).  Only two frames are defined by the rule."""
    if int(sampling_frame_num) != 2:
        raise ValueError("the interval rule selects two frames")
    n = int(video_length)
    interval = 4 if n <= 10 else 10 if n <= 20 else 15 if n <= 30 else 20 if n <= 40 else 36
    if n - interval <= 0:
        raise ValueError(f"a video of {n} frames is not longer than its interval {interval}")
    ref = int(rng.integers(0, n - interval))
    return [ref, ref + interval]


class VideoInstanceTrainMapper:
    """``YTVISDatasetMapper``, training branch, plus the model's normalisation, on clips whose frames are selected
    (:func:`sample_clip_frames`) and uploaded: a clip is ``(frames, annotations)``, ``frames`` a list of T uint8 (H, W,
    3) tensors and ``annotations`` a list of T lists of annotation dicts with an ``"id"`` (an annotation whose
    segmentation is None or empty counts as absent).  The views come from
    :func:`~bm2f_amd.train_mappers.video_clip_views` (its arguments are this class's config values).

    The instance ids of the selected frames are ordered ascending; the reference iterates a Python ``set`` there, whose
    order is the same for small non-negative integers and unspecified otherwise.  An instance absent from a frame is
    the dummy: class ``num_classes``, id -1, zero mask, zero box.  The video ``filter_empty_instances`` sets ``ids = -1``
    where the box is empty and removes nothing.  Returns per clip ``{"images" (T, 3, Hp, Wp), "instances": [per frame
    {"boxes", "labels", "ids", "masks" (G, Hc, Wc) uint8, "image_size"}], "views"}``, which ``prepare_video_targets`` and
    ``prepare_video_weaksup_targets`` take unchanged."""

    def __init__(self, *, min_sizes, max_size, sample_style, random_flip, augmentations, num_frames, num_classes,
                 pixel_mean, pixel_std, batch_divisibility=0, out_dtype=torch.float32):
        self.min_sizes, self.max_size, self.sample_style = min_sizes, int(max_size), sample_style
        self.random_flip, self.augmentations = random_flip, tuple(augmentations)
        self.num_frames, self.num_classes = int(num_frames), int(num_classes)
        self.pixel_mean, self.pixel_std = pixel_mean, pixel_std
        self.batch_divisibility = int(batch_divisibility)
        self.out_dtype = out_dtype

    def draw_views(self, clip_shapes, rng):
        """One list of views per clip (sources numbered within the clip)."""
        return [video_clip_views(shapes, min_sizes=self.min_sizes, max_size=self.max_size,
                                 sample_style=self.sample_style, random_flip=self.random_flip,
                                 augmentations=self.augmentations, clip_frame_cnt=self.num_frames, rng=rng)
                for shapes in clip_shapes]

    def __call__(self, clips, rng=None, views=None):
        rng = np.random.default_rng() if rng is None else rng
        T = self.num_frames
        for frames, anns in clips:
            if len(frames) != T or len(anns) != T:
                raise ValueError(f"a clip needs {T} frames and {T} annotation lists")
        frames = [f for c in clips for f in c[0]]
        shapes = [tuple(f.shape[:2]) for f in frames]
        if views is None:
            views = self.draw_views([shapes[b * T:(b + 1) * T] for b in range(len(clips))], rng)
        flat = [dataclasses.replace(v, source=b * T + t) for b, vs in enumerate(views) for t, v in enumerate(vs)]
        batch, sizes = image_views(frames, flat, pixel_mean=self.pixel_mean, pixel_std=self.pixel_std,
                                   out_dtype=self.out_dtype, size_divisibility=self.batch_divisibility)
        dev = batch.device
        # the clip's ids ascending; per frame one slot per id, absent ones the dummy
        segs, vos, slots, plans = [], [], [], []
        for b, (_, anns) in enumerate(clips):
            present = [{int(a["id"]): a for a in _kept(fa) if a.get("segmentation") is not None
                        and len(a["segmentation"]) > 0} for fa in anns]
            ids = sorted(set().union(*[set(p) for p in present]))
            plans.append((ids, present))
            for t in range(T):
                for g, i in enumerate(ids):
                    if i in present[t]:
                        segs.append(present[t][i]["segmentation"])
                        vos.append(b * T + t)
                        slots.append((b, t, g))
        masks, boxes, _ = view_masks(segs, vos, flat, shapes, dev, "uint8")
        where = {s: k for k, s in enumerate(slots)}
        out = []
        for b, (ids, present) in enumerate(plans):
            per_frame = []
            for t in range(T):
                Hc, Wc = sizes[b * T + t]
                rows = [where.get((b, t, g), -1) for g in range(len(ids))]
                have = torch.tensor([r >= 0 for r in rows], dtype=torch.bool, device=dev)
                idx = torch.tensor([max(r, 0) for r in rows], dtype=torch.int64, device=dev)
                if masks.shape[0]:
                    m = torch.where(have[:, None, None], masks[idx, :Hc, :Wc], 0)
                    bx = torch.where(have[:, None], boxes[idx], 0.0)
                else:
                    m = torch.zeros((len(ids), Hc, Wc), dtype=torch.uint8, device=dev)
                    bx = torch.zeros((len(ids), 4), dtype=torch.float32, device=dev)
                labels = torch.tensor([int(present[t][i]["category_id"]) if i in present[t] else self.num_classes
                                       for i in ids], dtype=torch.int64, device=dev)
                gid = torch.tensor([i if i in present[t] else -1 for i in ids], dtype=torch.int64, device=dev)
                nonempty = (bx[:, 2] - bx[:, 0] > 1e-5) & (bx[:, 3] - bx[:, 1] > 1e-5)
                per_frame.append({"boxes": bx, "labels": labels, "ids": torch.where(nonempty, gid, -1), "masks": m,
                                  "image_size": (Hc, Wc)})
            out.append({"images": batch[b * T:(b + 1) * T], "instances": per_frame, "views": views[b]})
        return out
