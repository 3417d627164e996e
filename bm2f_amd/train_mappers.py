"""Training mappers on the device: the reference's semantic, panoptic and video training views from uploaded tensors.

``MaskFormerSemanticDatasetMapper`` / ``MaskFormerPanopticDatasetMapper`` apply ``ResizeShortestEdge`` (a choice from
``MIN_SIZE_TRAIN``), a random crop, ``ColorAugSSDTransform`` and ``RandomFlip``, then pad image and label map to
``SIZE_DIVISIBILITY`` squared with 128 and the ignore label.  Here the random numbers are drawn on the host
(:func:`semantic_train_view`), and the pixels come from one ``image_views`` call (resize, crop, colour, flip, pad,
normalise, stack: one table upload, the colour stage inside the resize kernel) and one ``label_views`` call.  The
targets are ``semantic_targets`` / ``panoptic_targets`` of that label batch: label maps, no per-segment masks.

:func:`video_clip_views` restates ``mask2former_video/data_video/augmentation.py:build_augmentation``: the
``*_by_clip`` counters of its ``ResizeShortestEdge`` and ``RandomFlip`` and the brightness / contrast / saturation
blends drawn per frame.

Not claimed: the draws come from a ``numpy.random.Generator`` and follow the distributions and the order of the
reference's augmentation lists, not the bit stream of detectron2's ``random`` / ``np.random``; detectron2 and OpenCV were
never run against this module.  ``SINGLE_CATEGORY_MAX_AREA`` is 1.0 in every config of the reference, so
``RandomCrop_CategoryAreaConstraint`` is a plain random crop and its retry loop is not restated (a value below 1.0
is refused).  Out of scope as well: rotation (``cv2.warpAffine``), the video mappers' source-space ``T.RandomCrop``,
vertical flips and reading files.  Instance annotations (polygons, RLE, arrays) and the instance and video-instance
mappers are in :mod:`bm2f_amd.instance_mappers`.
"""
from __future__ import annotations

import numpy as np
import torch

from .color_aug import ColorAug, draw_color_aug_ssd, draw_video_photometric
from .image_views import View, image_views, label_views, resize_shortest_edge_size
from .label_targets import panoptic_targets, semantic_targets


def _crop_window(rh, rw, crop_type, crop_size, rng):
    """``T.RandomCrop(crop_type, crop_size)`` on an (rh, rw) image: (y0, x0, h, w)."""
    if crop_type == "absolute":
        ch, cw = min(int(crop_size[0]), rh), min(int(crop_size[1]), rw)
    elif crop_type == "relative":
        ch, cw = int(rh * crop_size[0] + 0.5), int(rw * crop_size[1] + 0.5)
    else:
        raise ValueError(f"crop type {crop_type!r} is not absolute or relative")
    if not (0 < ch <= rh and 0 < cw <= rw):
        raise ValueError(f"crop {(ch, cw)} does not fit the resized image {(rh, rw)}")
    return int(rng.integers(rh - ch + 1)), int(rng.integers(rw - cw + 1)), ch, cw


def semantic_train_view(h, w, *, min_sizes, max_size, crop_size, flip, color, rng, crop_type="absolute",
                        size_divisibility=0, img_format="BGR", source=0):
    """One training view of an (h, w) image, drawn in the semantic mapper's order: the short edge as a choice from
    ``min_sizes`` (through :func:`resize_shortest_edge_size`), the crop offset (``crop_size`` None: no crop), the
    colour (``color`` a :class:`ColorAug` to use, True to draw ``ColorAugSSDTransform`` for ``img_format``, None for
    none) and the flip coin (``flip`` False: no coin).  The canvas is ``size_divisibility`` squared when that is
    positive, as the mapper's ``F.pad`` makes it (a larger crop is cut there, as a negative pad cuts it), else the
    crop; fill 128."""
    size = int(rng.choice(np.asarray(min_sizes, dtype=np.int64)))
    rh, rw = resize_shortest_edge_size(h, w, size, max_size)
    crop = (0, 0, rh, rw) if crop_size is None else _crop_window(rh, rw, crop_type, crop_size, rng)
    if color is True:
        color = draw_color_aug_ssd(rng, img_format=img_format)
    elif color is False:
        color = None
    if color is not None and not isinstance(color, ColorAug):
        raise ValueError("color must be a ColorAug, True (draw ColorAugSSDTransform) or None")
    flip_out = bool(rng.random() < 0.5) if flip else False
    d = int(size_divisibility)
    return View(size=(rh, rw), source=source, crop=crop, canvas=(d, d) if d > 0 else crop[2:], flip_out=flip_out,
                fill=128, color=color)


class SemanticTrainMapper:
    """``MaskFormerSemanticDatasetMapper`` plus the model's normalisation, for a batch already on the device.

    Config values: ``min_sizes`` / ``max_size`` (``INPUT.MIN_SIZE_TRAIN`` / ``MAX_SIZE_TRAIN``, sampling "choice"),
    ``crop_size`` / ``crop_type`` (``INPUT.CROP.SIZE`` / ``TYPE``; None when ``CROP.ENABLED`` is off),
    ``single_category_max_area`` (only 1.0), ``color_aug_ssd``, ``img_format`` (``INPUT.FORMAT``),
    ``size_divisibility`` (``INPUT.SIZE_DIVISIBILITY``), ``ignore_label``, ``num_classes``, ``pixel_mean`` /
    ``pixel_std``; ``batch_divisibility`` is the model's ``ImageList.from_tensors`` rounding.

    ``mapper(samples, rng)`` takes a list of ``(image uint8 (H, W, 3), label map (H, W) uint8 / int16 / int32)`` tensors
    on one device and returns a dict: ``"images"`` the (B, 3, Hp, Wp) normalised batch, ``"image_sizes"``, ``"labels"``
    the (B, 1, Hp, Wp) label batch padded with the ignore label, ``"targets"`` (``semantic_targets`` of it) and
    ``"views"``."""

    def __init__(self, *, min_sizes, max_size, crop_size, ignore_label, num_classes, pixel_mean, pixel_std,
                 crop_type="absolute", single_category_max_area=1.0, color_aug_ssd=True, img_format="RGB",
                 size_divisibility=0, batch_divisibility=0, random_flip=True, out_dtype=torch.float32):
        if float(single_category_max_area) != 1.0:
            raise ValueError("SINGLE_CATEGORY_MAX_AREA below 1.0 (the retry loop of RandomCrop_CategoryAreaConstraint) "
                             "is out of scope")
        self.min_sizes = tuple(int(s) for s in min_sizes)
        if not self.min_sizes:
            raise ValueError("min_sizes is empty")
        self.max_size = int(max_size)
        self.crop_size = None if crop_size is None else tuple(crop_size)
        self.crop_type = crop_type
        self.color_aug_ssd = bool(color_aug_ssd)
        self.img_format = img_format
        self.size_divisibility = int(size_divisibility)
        self.batch_divisibility = int(batch_divisibility)
        self.ignore_label = int(ignore_label)
        self.num_classes = int(num_classes)
        self.pixel_mean, self.pixel_std = pixel_mean, pixel_std
        self.random_flip = bool(random_flip)
        self.out_dtype = out_dtype

    def draw_views(self, shapes, rng):
        return [semantic_train_view(h, w, min_sizes=self.min_sizes, max_size=self.max_size, crop_size=self.crop_size,
                                    crop_type=self.crop_type, flip=self.random_flip,
                                    color=True if self.color_aug_ssd else None, rng=rng,
                                    size_divisibility=self.size_divisibility, img_format=self.img_format, source=i)
                for i, (h, w) in enumerate(shapes)]

    def _views_and_batches(self, images, maps, rng, views, seg_pad):
        for im, m in zip(images, maps):
            if tuple(im.shape[:2]) != tuple(m.shape[-2:]):
                raise ValueError(f"image {tuple(im.shape[:2])} and label map {tuple(m.shape[-2:])} differ in size")
        if views is None:
            views = self.draw_views([tuple(im.shape[:2]) for im in images], rng)
        batch, sizes = image_views(images, views, pixel_mean=self.pixel_mean, pixel_std=self.pixel_std,
                                   out_dtype=self.out_dtype, size_divisibility=self.batch_divisibility)
        labels, _ = label_views(maps, views, seg_pad=seg_pad, size_divisibility=self.batch_divisibility)
        return views, batch, sizes, labels

    def __call__(self, samples, rng=None, views=None):
        rng = np.random.default_rng() if rng is None else rng
        images, maps = [s[0] for s in samples], [s[1] for s in samples]
        views, batch, sizes, labels = self._views_and_batches(images, maps, rng, views, self.ignore_label)
        targets = semantic_targets([labels[i, 0, :h, :w] for i, (h, w) in enumerate(sizes)], self.ignore_label,
                                   self.num_classes)
        return {"images": batch, "image_sizes": sizes, "labels": labels, "targets": targets, "views": views}


class PanopticTrainMapper(SemanticTrainMapper):
    """``MaskFormerPanopticDatasetMapper``: the semantic mapper's views on ``(image, panoptic id map (H, W) int32 after
    rgb2id, segments_info)`` samples.  The id map is padded with 0 (VOID), as the reference pads it; the targets are
    ``panoptic_targets`` of the label batch: every non-crowd segment of ``segments_info`` is kept, one that the crop
    left without pixels included, as the reference keeps it."""

    def __call__(self, samples, rng=None, views=None):
        rng = np.random.default_rng() if rng is None else rng
        images, maps, infos = [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples]
        views, batch, sizes, labels = self._views_and_batches(images, maps, rng, views, 0)
        targets = panoptic_targets([labels[i, 0, :h, :w] for i, (h, w) in enumerate(sizes)], infos)
        return {"images": batch, "image_sizes": sizes, "labels": labels, "targets": targets, "views": views}


def video_clip_views(shapes, *, min_sizes, max_size, sample_style, random_flip, augmentations, clip_frame_cnt, rng):
    """One :class:`View` per frame of ``shapes`` (a list of (h, w), frame i reading source i), as the training list of
    ``build_augmentation`` draws them: ``ResizeShortestEdge(min_sizes, max_size, sample_style)`` whose size is redrawn
    every ``clip_frame_cnt`` frames for the ``*_by_clip`` styles and every frame otherwise (``range``: an integer in
    ``[min_sizes[0], min_sizes[1]]``; ``choice``: one of ``min_sizes``); ``RandomFlip`` (``random_flip`` "none",
    "horizontal" per frame or "flip_by_clip" per clip); then the blends named in ``augmentations`` with a new weight
    per frame.  "vertical", "rotation" and ``INPUT.CROP`` are out of scope and raise."""
    if sample_style not in ("range", "choice", "range_by_clip", "choice_by_clip"):
        raise ValueError(f"sample_style {sample_style!r}")
    if random_flip not in ("none", "horizontal", "flip_by_clip"):
        raise ValueError(f"random_flip {random_flip!r} is not none, horizontal or flip_by_clip (vertical is out of scope)")
    min_sizes = (min_sizes, min_sizes) if isinstance(min_sizes, int) else tuple(int(s) for s in min_sizes)
    is_range = "range" in sample_style
    if is_range and len(min_sizes) != 2:
        raise ValueError("min_sizes must be two values for the range sample styles")
    size_every = int(clip_frame_cnt) if "by_clip" in sample_style else 1
    flip_every = int(clip_frame_cnt) if random_flip == "flip_by_clip" else 1
    if size_every <= 0 or flip_every <= 0:
        raise ValueError("clip_frame_cnt must be positive")
    names = [n for n in augmentations]
    views, size, flip = [], 0, False
    for i, (h, w) in enumerate(shapes):
        if i % size_every == 0:
            size = int(rng.integers(min_sizes[0], min_sizes[1] + 1)) if is_range else int(rng.choice(min_sizes))
        if random_flip != "none" and i % flip_every == 0:
            flip = bool(rng.random() < 0.5)
        color = draw_video_photometric(rng, names) if names else None
        hw = (int(h), int(w)) if size == 0 else resize_shortest_edge_size(h, w, size, max_size)     # size 0: NoOp
        views.append(View(size=hw, source=i, flip_out=flip, color=color if color is not None and color.ops else None))
    return views
