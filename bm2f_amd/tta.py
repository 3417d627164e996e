"""Semantic test-time augmentation: the reference's ``SemanticSegmentorWithTTA`` (test_time_augmentation.py).

The reference runs the model on every augmented view of an image (``TEST.AUG``: several ``MIN_SIZES``, each also
mirrored with ``FLIP``), takes each view's (K, H, W) ``sem_seg`` at the original size, flips it back where the view
was mirrored, adds it into a running sum and divides by the number of views (:71-98).  Here the model is still called
once per view, but it returns its *low-resolution* outputs (the triple :class:`MaskFormerInference` consumes) and the
head runs once over all views: ``m2f_infer_semantic_tta`` (``csrc/semantic_tta.hip``) extends the semantic head's GEMM
over the views, keeps the accumulators in registers and writes the (K, H, W) mean once -- or only its int16 argmax.

Both of the reference's orders are supported.  With ``before`` (``SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE``) a view's
logits are resized to the output and the sigmoid follows; without it (the default of the semantic configs) the view's
scores are computed on the crop and resized after.

On a CPU tensor :func:`semantic_inference_tta` restates the reference's loop literally in torch, so the semantics are
testable without a GPU.  That path is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.
"""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

from . import _native
from .inference import _MAX_K, _MAX_Q, _is_hip, _pair, _semantic_cpu, full_resolution_logits

_MAX_V = 32
_VIEW_FIELDS = 8   # include/bm2f.h: M2F_TTA_VIEW_FIELDS


def tta_view_sizes(height, width, min_sizes, max_size, flip=True):
    """The views of an (height, width) image as ``[(new_h, new_w, flipped)]``: for each of ``min_sizes`` the plain
    view, then (with ``flip``) the mirrored one.

    A restatement of detectron2's ``DatasetMapperTTA`` (one ``ResizeShortestEdge(size, max_size)`` per entry of
    ``TEST.AUG.MIN_SIZES``, then the same with a horizontal flip) and of ``ResizeShortestEdge.get_output_shape``:
    ``scale = size / min(h, w)``, the short side becomes ``size`` and the long side ``scale * long``; if the larger
    one exceeds ``max_size`` both are rescaled by ``max_size / larger``; each is then ``int(v + 0.5)``.  detectron2 is
    not installed where this was written and has not been run against it; the values the tests pin are worked by hand.
    """
    h, w = int(height), int(width)
    if h <= 0 or w <= 0:
        raise ValueError(f"image size {(h, w)} must be positive")
    views = []
    for size in min_sizes:
        size = float(size)
        scale = size / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > max_size:
            scale = max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        shape = (int(newh + 0.5), int(neww + 0.5))
        views.append((*shape, False))
        if flip:
            views.append((*shape, True))
    return views


def _check_views(views, num_classes):
    """-> [(pred_logits (Q, K+1), pred_masks (Q, h, w), (Hp, Wp), (Hc, Wc), flipped)], validated."""
    V = len(views)
    if not 1 <= V <= _MAX_V:
        raise ValueError(f"{V} views outside [1, {_MAX_V}]")
    out = []
    for outputs, padded_size, image_size, flipped in views:
        cls, masks = outputs["pred_logits"], outputs["pred_masks"]
        if cls.dim() != 2 or masks.dim() != 3:
            raise ValueError("a view's pred_logits must be (Q, K+1) and its pred_masks (Q, h, w)")
        (Hp, Wp), (Hc, Wc) = _pair(padded_size), _pair(image_size)
        if not (0 < Hc <= Hp and 0 < Wc <= Wp):
            raise ValueError(f"image size {(Hc, Wc)} does not fit the padded size {(Hp, Wp)}")
        out.append((cls, masks, (Hp, Wp), (Hc, Wc), bool(flipped)))
    cls0, masks0 = out[0][:2]
    Q = masks0.shape[0]
    if cls0.shape[1] != num_classes + 1:
        raise ValueError(f"pred_logits has {cls0.shape[1]} columns, expected num_classes + 1")
    if not 0 < num_classes <= _MAX_K:
        raise ValueError(f"num_classes {num_classes} outside [1, {_MAX_K}]")
    if not 0 < Q <= _MAX_Q:
        raise ValueError(f"{Q} queries outside [1, {_MAX_Q}]")
    for cls, masks, *_ in out:
        if cls.shape != cls0.shape or masks.shape[0] != Q or cls.shape[0] != Q:
            raise ValueError("the views differ in their number of queries or classes")
        if masks.dtype != masks0.dtype or cls.dtype != cls0.dtype:
            raise ValueError("the views differ in dtype")
        if masks.device != masks0.device or cls.device != masks0.device:
            raise ValueError("the views lie on different devices")
    return out


def _tta_cpu(views, out_size, before):
    """test_time_augmentation.py:78-98 on the eval branch of MaskFormer.forward (maskformer_model.py:337-364)."""
    total = None
    for cls, masks, padded, image, flipped in views:
        if before:
            r = _semantic_cpu(cls, full_resolution_logits(masks, padded, image, out_size))
        else:
            r = _semantic_cpu(cls, full_resolution_logits(masks, padded, image))
            if tuple(r.shape[-2:]) != out_size:
                r = F.interpolate(r[None], size=out_size, mode="bilinear", align_corners=False)[0]
        if flipped:
            r = r.flip(dims=[2])
        total = r if total is None else total + r
    return total / len(views)


def _logit_span(masks):
    """The views' logits, left where they are, as one address range: (base pointer, elements, element offset per
    view, the tensors to keep alive over the launch)."""
    masks = [m.detach().contiguous() for m in masks]
    size = masks[0].element_size()
    base = min(m.data_ptr() for m in masks)
    if any((m.data_ptr() - base) % size for m in masks):
        raise ValueError("the views' pred_masks are not aligned to their element size")
    end = max(m.data_ptr() + m.numel() * size for m in masks)
    return base, (end - base) // size, [(m.data_ptr() - base) // size for m in masks], masks


def _tta_hip(views, out_size, before, labels):
    """No copy of the logits, one (V, K, Q) probs tensor, one upload of the view table, one launch."""
    dev = views[0][1].device
    V, Q = len(views), views[0][1].shape[0]
    base, numel, offs, keep = _logit_span([v[1] for v in views])
    probs = F.softmax(torch.stack([v[0] for v in views]).float(), dim=-1)[..., :-1].transpose(1, 2).contiguous()
    K = probs.shape[1]
    rows = [(off, *masks.shape[-2:], Hp, Wp, Hc, Wc, int(flipped))
            for off, (_, masks, (Hp, Wp), (Hc, Wc), flipped) in zip(offs, views)]
    table = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
    assert table.shape[1] == _VIEW_FIELDS
    Ho, Wo = out_size
    if labels:
        out = torch.empty((Ho, Wo), dtype=torch.int16, device=dev)
        sem_ptr, lab_ptr = None, out.data_ptr()
    else:
        out = torch.empty((K, Ho, Wo), dtype=torch.float32, device=dev)
        sem_ptr, lab_ptr = out.data_ptr(), None
    _native.call("m2f_infer_semantic_tta", base, _native.dtype_code(views[0][1].dtype, "TTA masks"), numel,
                 probs.data_ptr(), table.data_ptr(), V, Q, K, Ho, Wo, int(bool(before)), sem_ptr, lab_ptr,
                 _native.stream(dev))
    del keep
    return out


def semantic_inference_tta(views, output_size, *, num_classes, before=False, labels=False):
    """The mean semantic scores of one image over its augmented views.

    views: a list of ``(outputs, padded_size, image_size, flipped)``, one per view, with ``outputs =
    {"pred_logits": (Q, K+1), "pred_masks": (Q, h, w)}`` the decoder's low-resolution outputs for that view,
    ``padded_size`` the (Hp, Wp) its batch was padded to, ``image_size`` the view's own (Hc, Wc) and ``flipped``
    whether the view was mirrored horizontally.  output_size: the (height, width) of the original image.

    Returns the (K, height, width) fp32 mean, or with ``labels`` its (height, width) int16 argmax.  ``before``
    selects ``sem_seg_postprocess_before_inference``.  On a HIP tensor this is one upload of the view table and one
    kernel launch, and with ``labels`` no (K, height, width) tensor is allocated; 16-bit mask logits are converted to
    fp32 on load.  On a CPU tensor it is the reference's loop in torch.  Raises ValueError on mixed dtypes or devices,
    on a view count outside [1, 32] and on K or Q mismatches between the views."""
    views = _check_views(list(views), int(num_classes))
    out_size = _pair(output_size)
    if out_size[0] <= 0 or out_size[1] <= 0:
        raise ValueError(f"output size {out_size} must be positive")
    if _is_hip(views[0][1]):
        return _tta_hip(views, out_size, before, labels)
    r = _tta_cpu(views, out_size, before)
    return r.argmax(0).to(torch.int16) if labels else r


def _is_flipped(view):
    """A view dict marks a mirrored image with ``"flipped"``, or as detectron2's mapper does, with an ``HFlipTransform``
    in its ``"transforms"`` list (matched by class name: fvcore is not a dependency)."""
    if "flipped" in view:
        return bool(view["flipped"])
    tfms = view.get("transforms")
    return any(type(t).__name__ == "HFlipTransform" for t in getattr(tfms, "transforms", tfms or ()))


class SemanticSegmentorWithTTA:
    """``SemanticSegmentorWithTTA`` of the reference on the fused multi-view head.

    model: a callable that takes ``[view_dict]`` and returns ``(outputs, padded_size, image_sizes)`` for that batch of
    one, the triple :meth:`MaskFormerInference.forward` consumes (``outputs["pred_masks"]`` is (1, Q, h, w)).  It is
    called once per view, as in the reference; the head then runs once over all views.

    tta_mapper: a callable that takes the input dict (with ``"image"``, ``"height"``, ``"width"``) and returns the list
    of view dicts, each with its ``"image"`` and either ``"flipped"`` or detectron2's ``"transforms"``.  The default
    mapper sizes the views with :func:`tta_view_sizes` from (height, width), resizes ``"image"`` on its own device
    with ``F.interpolate(mode="bilinear", antialias=True)`` and mirrors it with ``.flip(-1)``.  That is not PIL's
    arithmetic, which the reference's host mapper uses: a caller who wants the reference's exact pixels passes its own
    ``tta_mapper``.  Reading the image from ``"file_name"`` is out of scope: an input without ``"image"`` raises.
    """

    def __init__(self, model, *, num_classes, min_sizes, max_size, flip=True, before=False, tta_mapper=None,
                 semantic_labels=False):
        if not 0 < num_classes <= _MAX_K:
            raise ValueError(f"num_classes {num_classes} outside [1, {_MAX_K}]")
        self.model = model
        self.num_classes = int(num_classes)
        self.min_sizes = tuple(int(s) for s in min_sizes)
        self.max_size = int(max_size)
        self.flip = bool(flip)
        self.before = bool(before)
        self.tta_mapper = tta_mapper if tta_mapper is not None else self._default_mapper
        self.semantic_labels = bool(semantic_labels)
        if tta_mapper is None and not 1 <= len(self.min_sizes) * (2 if self.flip else 1) <= _MAX_V:
            raise ValueError(f"min_sizes and flip give a view count outside [1, {_MAX_V}]")

    @classmethod
    def from_config(cls, cfg, model, **kw):
        aug = cfg.TEST.AUG
        return cls(model, num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, min_sizes=aug.MIN_SIZES,
                   max_size=aug.MAX_SIZE, flip=aug.FLIP,
                   before=cfg.MODEL.MASK_FORMER.TEST.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE, **kw)

    def _default_mapper(self, x):
        image = x["image"]
        views = []
        for newh, neww, flipped in tta_view_sizes(x["height"], x["width"], self.min_sizes, self.max_size, self.flip):
            img = image[None] if image.is_floating_point() else image[None].float()
            img = F.interpolate(img, size=(newh, neww), mode="bilinear", align_corners=False, antialias=True)[0]
            view = copy.copy(x)
            view["image"] = img.flip(-1) if flipped else img
            view["flipped"] = flipped
            views.append(view)
        return views

    def __call__(self, batched_inputs):
        """Same input / output format as the reference: per input ``{"sem_seg": (K, height, width)}``, or with
        ``semantic_labels`` ``{"sem_seg_labels": (height, width) int16}``."""
        results = []
        for x in batched_inputs:
            if "image" not in x:
                raise ValueError("SemanticSegmentorWithTTA needs the \"image\" tensor; it does not read files")
            x = copy.copy(x)
            if "height" not in x and "width" not in x:     # test_time_augmentation.py:60-62
                x["height"], x["width"] = (int(s) for s in x["image"].shape[-2:])
            results.append(self._inference_one_image(x))
        return results

    def _inference_one_image(self, x):
        views = []
        with torch.no_grad():
            for view in self.tta_mapper(x):
                flipped = _is_flipped(view)
                view = {k: v for k, v in view.items() if k not in ("transforms", "flipped")}
                outputs, padded_size, image_sizes = self.model([view])
                if outputs["pred_masks"].shape[0] != 1 or len(image_sizes) != 1:
                    raise ValueError("the model must return a batch of one per view")
                views.append(({"pred_logits": outputs["pred_logits"][0], "pred_masks": outputs["pred_masks"][0]},
                              padded_size, image_sizes[0], flipped))
            r = semantic_inference_tta(views, (x["height"], x["width"]), num_classes=self.num_classes,
                                       before=self.before, labels=self.semantic_labels)
        return {"sem_seg_labels" if self.semantic_labels else "sem_seg": r}
