"""The reference's photometric augmentations as definitions on uint8 (H, W, 3) numpy arrays.

Two families.  detectron2's ``ColorAugSSDTransform`` (``COLOR_AUG_SSD: True`` in every ``Base-*`` config of ADE20K,
Cityscapes and Mapillary Vistas): brightness, then contrast / saturation / hue in one of two orders, each step present or
absent, saturation and hue through OpenCV's 8-bit HSV.  And the ``INPUT.AUGMENTATIONS`` of
``mask2former_video/data_video/augmentation.py``: ``RandomBrightness`` / ``RandomContrast`` / ``RandomSaturation``,
which are ``BlendTransform`` s.  The functions here are the specification: ``m2f_image_views_color``
(``csrc/image_views.hip``) must equal them bit for bit, and ``image_views`` runs them itself on CPU tensors.

What has and has not been checked.  **This restatement has not been run against cv2 or detectron2**: neither is
installed where it was written.  The HSV conversion is written from OpenCV's ``imgproc`` colour code (the integer
``BGR2HSV`` with its two division tables, the fp32 ``HSV2BGR`` with its sector table); tests hold it to anchors and
invariants, not to OpenCV's output.  The blends are held to the literal numpy expressions of ``BlendTransform`` under
the installed numpy (tests/test_color_aug_cpu.py); NumPy 2 promotion gives fp32 for brightness (a Python float is a
weak scalar) and fp64 for contrast and saturation (``img.mean()`` and ``img.dot(...)`` are fp64 values).  The draw
helpers follow detectron2's distributions; parity of the *sequence* of draws with detectron2's use of ``random`` /
``np.random`` is not claimed.

Every fp32 and fp64 operation below is rounded on its own: there is no fused multiply-add except the one spelled out
in :func:`grayscale`.
"""
from __future__ import annotations

import dataclasses

import numpy as np

MAX_OPS = 4                 # include/bm2f.h: M2F_COLOR_MAX_OPS
FIELDS = 16                 # include/bm2f.h: M2F_COLOR_FIELDS
_CONVERT, _SSD_SAT, _SSD_HUE, _CONTRAST, _SATURATION = 1, 2, 3, 4, 5     # include/bm2f.h: M2F_COLOR_*
_HSV_SHIFT = 12
_F32 = np.float32
GRAY_WEIGHTS = (0.299, 0.587, 0.114)
OP_NAMES = ("ssd_brightness", "ssd_contrast", "ssd_saturation", "ssd_hue", "brightness", "contrast", "saturation")


@dataclasses.dataclass(frozen=True)
class ColorAug:
    """An ordered list of photometric operations with their drawn parameters.

    ops: tuples ``(name, value)``: ``("ssd_brightness", delta)``, ``("ssd_contrast", alpha)``, ``("ssd_saturation",
    alpha)``, ``("ssd_hue", int delta)`` and the blends ``("brightness", w)``, ``("contrast", w)``, ``("saturation",
    w)``.  At most ``MAX_OPS`` operations and at most one ``"contrast"`` (its mean is one number per view).
    swap_rb: the operations see channels 2, 1, 0 (``ColorAugSSDTransform`` on ``FORMAT: "RGB"``, which works on BGR).
    """
    ops: tuple = ()
    swap_rb: bool = False

    def __post_init__(self):
        ops = tuple((str(n), (int(v) if n == "ssd_hue" else float(v))) for n, v in self.ops)
        object.__setattr__(self, "ops", ops)
        object.__setattr__(self, "swap_rb", bool(self.swap_rb))
        for n, _ in ops:
            if n not in OP_NAMES:
                raise ValueError(f"unknown colour operation {n!r}; known: {OP_NAMES}")
        if len(ops) > MAX_OPS:
            raise ValueError(f"{len(ops)} colour operations; at most {MAX_OPS} per view")
        if sum(n == "contrast" for n, _ in ops) > 1:
            raise ValueError("at most one \"contrast\" blend per view")

    @property
    def contrast_index(self):
        """Position of the ``"contrast"`` blend, -1 without one."""
        return next((i for i, (n, _) in enumerate(self.ops) if n == "contrast"), -1)

    @property
    def needs_hsv(self):
        return any(n in ("ssd_saturation", "ssd_hue") for n, _ in self.ops)


# ------------------------------------------------------------------------------------------------ SSD
def _u8(img):
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f"a colour operation takes uint8, got {img.dtype}")
    return img


def convert(img, alpha=1, beta=0):
    """``ColorAugSSDTransform.convert``: ``img.astype(float32) * alpha + beta`` in fp32 (alpha and beta rounded to
    fp32, the product and the sum rounded separately), clipped to [0, 255], truncated to uint8."""
    x = _u8(img).astype(_F32) * _F32(alpha)
    x = x + _F32(beta)
    return np.clip(x, _F32(0), _F32(255)).astype(np.uint8)


def ssd_brightness(img, delta):
    return convert(img, beta=delta)


def ssd_contrast(img, alpha):
    return convert(img, alpha=alpha)


def hsv_tables():
    """OpenCV's ``sdiv_table`` and ``hdiv_table180`` (256 int32 each): ``rint((255 << 12) / i)`` and ``rint((180 << 12)
    / (6 i))`` in fp64, 0 at i = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, dtype=np.int32)
    hdiv = np.zeros(256, dtype=np.int32)
    sdiv[1:] = np.rint((255 << _HSV_SHIFT) / i).astype(np.int32)
    hdiv[1:] = np.rint((180 << _HSV_SHIFT) / (6.0 * i)).astype(np.int32)
    return sdiv, hdiv


_SDIV, _HDIV = hsv_tables()


def bgr2hsv(img):
    """``cv2.cvtColor(img, COLOR_BGR2HSV)`` on uint8: H in [0, 180), integer arithmetic."""
    p = _u8(img).astype(np.int32)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    half = 1 << (_HSV_SHIFT - 1)
    s = (diff * _SDIV[v] + half) >> _HSV_SHIFT
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h0 * _HDIV[diff] + half) >> _HSV_SHIFT             # arithmetic shift: h0 may be negative
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), s, v], axis=-1).astype(np.uint8)


_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
_HSCALE = _F32(6) / _F32(180)


def hsv2bgr(img):
    """``cv2.cvtColor(img, COLOR_HSV2BGR)`` on uint8 (H in [0, 180)): fp32 on h, s / 255 and v / 255, the result
    ``rint(x * 255)`` (ties to even) saturated to a byte."""
    p = _u8(img)
    one = _F32(1)
    h = p[..., 0].astype(_F32) * _HSCALE
    s = p[..., 1].astype(_F32) / _F32(255)
    v = p[..., 2].astype(_F32) / _F32(255)
    sector = np.floor(h)
    h = h - sector
    sector = sector.astype(np.int64)
    outside = (sector < 0) | (sector > 5)
    sector = np.where(outside, 0, sector)
    h = np.where(outside, _F32(0), h)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    bgr = np.take_along_axis(tab, _SECTORS[sector], axis=-1)
    bgr = np.where((p[..., 1] == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * _F32(255)), 0, 255).astype(np.uint8)


def ssd_saturation(img, alpha):
    hsv = bgr2hsv(img)
    hsv[..., 1] = convert(hsv[..., 1], alpha=alpha)
    return hsv2bgr(hsv)


def ssd_hue(img, delta):
    hsv = bgr2hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(delta)) % 180).astype(np.uint8)     # Python's modulo: >= 0
    return hsv2bgr(hsv)


# ------------------------------------------------------------------------------------------------ video blends
def _blend64(src, src_weight, dst_weight, img):
    """``clip(src_weight * src + dst_weight * img.astype(float32), 0, 255).astype(uint8)`` for an fp64 ``src``: the
    first product in fp64, the second in fp32 (dst_weight rounded to fp32), their sum in fp64."""
    x = np.float64(src_weight) * np.asarray(src, dtype=np.float64)
    y = (_F32(dst_weight) * img.astype(_F32)).astype(np.float64)
    return np.clip(x + y, 0.0, 255.0).astype(np.uint8)


def blend_brightness(img, w):
    """``RandomBrightness``: ``BlendTransform(src_image=0, src_weight=1 - w, dst_weight=w)``; fp32 throughout, so it is
    ``convert(alpha=w, beta=(1 - w) * 0)``."""
    return convert(img, alpha=w, beta=(1 - float(w)) * 0)


def exact_mean(total, count):
    """``img.mean()`` of a uint8 array from its exact integer sum: one fp64 division."""
    return np.float64(int(total)) / np.float64(int(count))


def blend_contrast(img, w, mean=None):
    """``RandomContrast``: ``src_image = img.mean()``, the fp64 mean over all three channels (of ``img`` unless
    ``mean`` is given)."""
    img = _u8(img)
    if mean is None:
        mean = exact_mean(img.sum(dtype=np.int64), img.size)
    return _blend64(mean, 1 - float(w), w, img)


def _mantissa(x, bits):
    m = x * 2.0 ** bits
    assert m == int(m) and int(m) < 1 << 56
    return np.uint64(int(m))


def grayscale(img):
    """``img.dot([0.299, 0.587, 0.114])`` as the installed numpy evaluates it, (H, W) fp64: the BLAS kernel behind
    ``dot`` accumulates with fused multiply-adds, ``fma(c2, 0.114, fma(c1, 0.587, c0 * 0.299))``, two roundings fewer
    than three products and two sums.  The chain is reproduced exactly in 64-bit integers in units of 2^-56 (every
    value is below 256 = 2^64 * 2^-56), each rounding being the integer -> fp64 conversion."""
    p = _u8(img)
    w0, w1, w2 = GRAY_WEIGHTS
    unit = 2.0 ** 56
    t = p[..., 0].astype(np.float64) * w0                                        # one rounding
    acc = p[..., 1].astype(np.uint64) * _mantissa(w1, 56) + (t * unit).astype(np.uint64)
    t = acc.astype(np.float64)                                                   # the first fma's rounding
    acc = p[..., 2].astype(np.uint64) * _mantissa(w2, 56) + t.astype(np.uint64)
    return acc.astype(np.float64) / unit                                         # the second's; the scale is exact


def blend_saturation(img, w):
    """``RandomSaturation``: ``src_image = img.dot([0.299, 0.587, 0.114])[..., None]`` on the channels as stored."""
    img = _u8(img)
    return _blend64(grayscale(img)[..., None], 1 - float(w), w, img)


# ------------------------------------------------------------------------------------------------ composition
_STEP = {"ssd_brightness": ssd_brightness, "ssd_contrast": ssd_contrast, "ssd_saturation": ssd_saturation,
         "ssd_hue": ssd_hue, "brightness": blend_brightness, "contrast": blend_contrast,
         "saturation": blend_saturation}


def apply_color(img, aug):
    """All operations of ``aug`` on a uint8 (..., 3) array of the pixels a view shows; the contrast mean is over
    exactly these pixels, after the operations before it."""
    img = _u8(img)
    if aug is None or not aug.ops or img.size == 0:
        return img
    x = img[..., ::-1] if aug.swap_rb else img
    for name, value in aug.ops:
        x = _STEP[name](x, value)
    return np.ascontiguousarray(x[..., ::-1] if aug.swap_rb else x)


def color_sum(img, aug):
    """The exact integer sum the contrast blend of ``aug`` takes its mean from (what ``m2f_image_views_sum`` writes)."""
    x = _u8(img)[..., ::-1] if aug.swap_rb else _u8(img)
    for name, value in aug.ops[:max(aug.contrast_index, 0)]:
        x = _STEP[name](x, value)
    return int(x.sum(dtype=np.int64))


def encode(aug):
    """One row of the kernel's colour table (``FIELDS`` fp64, include/bm2f.h): n, swap_rb, contrast index, 0, then
    per operation (code, a, b).  The SSD brightness / contrast and the brightness blend are all ``convert``."""
    row = np.zeros(FIELDS, dtype=np.float64)
    if aug is None:
        row[2] = -1
        return row
    row[0], row[1], row[2] = len(aug.ops), int(aug.swap_rb), aug.contrast_index
    for k, (name, v) in enumerate(aug.ops):
        row[4 + 3 * k:7 + 3 * k] = {
            "ssd_brightness": (_CONVERT, 1.0, v), "ssd_contrast": (_CONVERT, v, 0.0),
            "brightness": (_CONVERT, v, (1 - v) * 0), "ssd_saturation": (_SSD_SAT, v, 0.0),
            "ssd_hue": (_SSD_HUE, v, 0.0), "contrast": (_CONTRAST, 1 - v, v), "saturation": (_SATURATION, 1 - v, v),
        }[name]
    return row


# ------------------------------------------------------------------------------------------------ draws
def draw_color_aug_ssd(rng, brightness_delta=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue_delta=18,
                       img_format="BGR"):
    """One draw of ``ColorAugSSDTransform``: each step with probability 1/2; brightness ``uniform(-delta, delta)``,
    contrast and saturation ``uniform(low, high)``, hue an integer in ``[-hue_delta, hue_delta]``; brightness first,
    then with probability 1/2 contrast, saturation, hue, else saturation, hue, contrast.  ``rng`` is a
    ``numpy.random.Generator``; detectron2 draws from ``random``, and the sequence of draws is not reproduced."""
    if img_format not in ("BGR", "RGB"):
        raise ValueError(f"img_format {img_format!r} is not BGR or RGB")
    ops = []

    def maybe(name, draw):
        if int(rng.integers(2)):
            ops.append((name, draw()))

    def sat_hue():
        maybe("ssd_saturation", lambda: float(rng.uniform(*saturation)))
        maybe("ssd_hue", lambda: int(rng.integers(-hue_delta, hue_delta + 1)))

    def con():
        maybe("ssd_contrast", lambda: float(rng.uniform(*contrast)))

    maybe("ssd_brightness", lambda: float(rng.uniform(-brightness_delta, brightness_delta)))
    if int(rng.integers(2)):
        con()
        sat_hue()
    else:
        sat_hue()
        con()
    return ColorAug(tuple(ops), swap_rb=img_format == "RGB")


def draw_video_photometric(rng, names, low=0.9, high=1.1):
    """The blends of ``build_augmentation`` for ``INPUT.AUGMENTATIONS = names``: brightness, contrast, saturation in
    this order, each with ``w = uniform(low, high)`` (``T.RandomBrightness(0.9, 1.1)`` ...).  ``"rotation"`` is out
    of scope and raises."""
    names = list(names)
    for n in names:
        if n not in ("brightness", "contrast", "saturation"):
            raise ValueError(f"augmentation {n!r} is not brightness, contrast or saturation (rotation is out of scope)")
    return ColorAug(tuple((n, float(rng.uniform(low, high))) for n in ("brightness", "contrast", "saturation")
                          if n in names))
