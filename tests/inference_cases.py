"""Synthetic cases for the image inference heads (csrc/inference.hip), shared by test_inference_sweep_cpu.py and
test_inference_sweep_gpu.py.  A case is the SimpleNamespace ``inference_util.load()`` returns, so ``iu.module``,
``iu.expected_from_cpu`` and the ``iu.check_*`` bars apply unchanged; the expectation is the CPU path plus the
fp64 ambiguity maps, no golden file.

Inputs (seeded ``torch.Generator``; plain randn keeps almost no query and yields no segment):
  class logits  randn * 2 over K + 1 columns, then by role: "kept" queries get one favoured class at probability
                0.9 .. 0.96 (owners, below: 0.998), "void" queries favour "no object", the rest stay spread out (non-void, below the
                object-mask threshold).  ``cls_ramp`` is a second table for the semantic head alone: probability
                proportional to k + 1, so every class plane differs from every other by max / K > the bar and a
                permuted class index cannot pass.
  mask logits   low-frequency blobs (amplitude 3) plus noise 0.5.  Up to four kept queries are "owners": +5 inside
                their stripe of the logit map and -5 outside, so they win real area; the first two share one stuff
                class (a merge), the others are things.  Kept non-owners win only scraps of their own positive area
                (dropped by the overlap threshold).

The thresholds are the fixture's (0.8, 0.8): the fp64 evaluation in gen_inference_golden.py has them built in.
K = 1 is not covered: that evaluation takes a top-2 over classes.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import inference_util as iu

THRESHOLDS = (0.8, 0.8)
INF = float("inf")
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
K_SWEEP = (2, 31, 32, 33, 64, 65, 96, 128, 150, 171, 192, 224, 225, 256)
Q_SWEEP = (1, 31, 32, 33, 64, 100, 200, 256)
WIDTHS = (1, 31, 32, 33, 63, 64, 65)     # at height 5
HEIGHTS = (1, 3, 4)                      # at width 33 (height 5 is WIDTHS' 33)
SOURCES = ((1, 7), (7, 1), (2, 2))       # degenerate logit maps, to 16 x 16


def synth(name, *, Q, K, hw, padded, image_sizes, output_sizes, seed, things, topk, keep="some", twins=False,
          inf=False):
    g = torch.Generator().manual_seed(seed)
    B, (h, w) = len(image_sizes), hw
    cls = torch.randn(B, Q, K + 1, generator=g) * 2
    low = torch.randn(B, Q, (h + 2) // 3 + 1, (w + 2) // 3 + 1, generator=g)
    masks = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=True) * 3
    masks = masks + torch.randn(B, Q, h, w, generator=g) * 0.5
    n_kept = {"some": max(1, (3 * Q + 9) // 10), "all": Q, "none": 0}[keep]
    n_void = Q - n_kept if keep == "none" else min(Q - n_kept, (3 * Q) // 10)
    stuff = list(range(things, K)) or list(range(K))
    thing = list(range(things)) or stuff
    along_w = w >= h
    L = w if along_w else h
    for b in range(B):
        order = torch.randperm(Q, generator=g).tolist()
        kept, void = sorted(order[:n_kept]), order[n_kept:n_kept + n_void]
        owners = kept[:min(len(kept), 4, L)]
        prob = (0.81 + 0.02 * torch.rand(Q, generator=g)) if twins else (0.9 + 0.06 * torch.rand(Q, generator=g))
        fav = torch.randint(0, K, (Q,), generator=g)
        for q in kept:
            t = owners.index(q) if q in owners else -1
            k = int(fav[q]) if t < 0 else (stuff[0] if t < 2 else thing[(t - 2) % len(thing)])
            p = 0.998 if t >= 0 else float(prob[q])
            rest = torch.cat([cls[b, q, :k], cls[b, q, k + 1:]]).exp().sum()
            cls[b, q, k] = torch.log(rest * p / (1 - p))
        for q in void:
            cls[b, q, K] = torch.log(cls[b, q, :K].exp().sum() * 19)
        stripes = max(2, len(owners))
        stripe = torch.arange(L) * stripes // L
        stripe = stripe[None, :].expand(h, w) if along_w else stripe[:, None].expand(h, w)
        for t, q in enumerate(owners):
            masks[b, q] = torch.where(stripe == t, 5.0, -5.0) + torch.randn(h, w, generator=g) * 0.5
        if twins:
            # an exact copy of the first owner (a thing here, at 0.9 above the other kept queries' 0.81 .. 0.83): equal
            # scores at every pixel, the first one wins.  The other three owners' 0.998 fill the instance head's
            # top-k of 3, which so takes neither twin (equal instance scores could not be paired)
            a, c2 = owners[0], kept[-1]
            for q in (a, c2):
                k, p = thing[2 % len(thing)], 0.9
                cls[b, q] = cls[b, a]
                cls[b, q, K] = -20.0
                rest = torch.cat([cls[b, q, :k], cls[b, q, k + 1:]]).exp().sum()
                cls[b, q, k] = torch.log(rest * p / (1 - p))
            cls[b, c2] = cls[b, a]
            masks[b, c2] = masks[b, a]
    if inf:
        # isolated infinite texels, away from row / column 1 (the only texels a 4x upscale reads with weight 0, at
        # the clamped border): the full-resolution logits hold +-inf but no NaN
        assert (h, w) == (6, 10) and Q >= 3
        own = sorted(order[:n_kept])[0]
        masks[:, own, 4, 6], masks[:, order[-1], 3, 4], masks[:, order[-2], 2, 7] = INF, INF, -INF
    ramp = torch.log(torch.arange(1, K + 2, dtype=torch.float32)).repeat(B, Q, 1)
    ramp[..., K] = torch.log(torch.rand(B, Q, generator=g) * K + 1)
    return SimpleNamespace(name=name, Q=Q, K=K, things=things, topk=topk, padded=tuple(padded),
                           image_sizes=[tuple(s) for s in image_sizes], output_sizes=[tuple(s) for s in output_sizes],
                           thresholds=THRESHOLDS, B=B, cls=cls, masks=masks, cls_ramp=ramp, twins=twins)


_UP = dict(hw=(6, 10), padded=(24, 40), image_sizes=[(24, 40)], output_sizes=[(24, 40)])
_DOWN = dict(Q=40, K=9, things=4, topk=20, hw=(40, 72), padded=(40, 72))
_SMALL = dict(Q=5, K=3, things=2, topk=15)          # topk == Q * K
_SPECS = {}
for _k in K_SWEEP:
    _SPECS[f"K{_k}"] = dict(Q=33, K=_k, things=_k // 2, topk=min(20, 33 * _k), seed=100 + _k, **_UP)
for _q in Q_SWEEP:
    _SPECS[f"Q{_q}"] = dict(Q=_q, K=40, things=20, topk=20, seed=400 + _q, keep="all" if _q == 256 else "some", **_UP)
_SPECS["direct"] = dict(seed=1, image_sizes=[(40, 72)], output_sizes=[(19, 35)], **_DOWN)
_SPECS["mixed"] = dict(seed=2, image_sizes=[(40, 72), (40, 72)], output_sizes=[(19, 35), (40, 72)], **_DOWN)
_SPECS["mixed_sizes"] = dict(seed=3, image_sizes=[(40, 72), (33, 61)], output_sizes=[(19, 35), (50, 90)], **_DOWN)
for _w in WIDTHS:
    _SPECS[f"w{_w}"] = dict(seed=600 + _w, hw=(4, 6), padded=(16, 24), image_sizes=[(13, 21)],
                            output_sizes=[(5, _w)], **_SMALL)
for _h in HEIGHTS:
    _SPECS[f"h{_h}"] = dict(seed=700 + _h, hw=(4, 6), padded=(16, 24), image_sizes=[(13, 21)],
                            output_sizes=[(_h, 33)], **_SMALL)
_SPECS["out32x32"] = dict(seed=11, hw=(8, 8), padded=(32, 32), image_sizes=[(32, 32)], output_sizes=[(32, 32)], **_SMALL)
_SPECS["out25x41"] = dict(seed=12, hw=(8, 8), padded=(32, 32), image_sizes=[(32, 32)], output_sizes=[(25, 41)], **_SMALL)
for _s in SOURCES:
    _SPECS["src%dx%d" % _s] = dict(seed=800 + 10 * _s[0] + _s[1], hw=_s, padded=(16, 16), image_sizes=[(16, 16)],
                                   output_sizes=[(16, 16)], **_SMALL)
_SPECS["many_tiles"] = dict(seed=21, hw=(17, 17), padded=(68, 68), image_sizes=[(68, 68)], output_sizes=[(262, 259)],
                            **_SMALL)
_SPECS["none_kept"] = dict(Q=33, K=40, things=20, topk=20, seed=31, keep="none", **_UP)
_SPECS["no_things"] = dict(Q=33, K=40, things=0, topk=20, seed=32, **_UP)
_SPECS["twins"] = dict(Q=33, K=40, things=20, topk=3, seed=33, twins=True, **_UP)

_SPECS["inf"] = dict(Q=33, K=40, things=20, topk=20, seed=34, inf=True, **_UP)
_SPECS["nan_clean"] = dict(Q=33, K=40, things=20, topk=20, seed=35, **_UP)

NAMES = tuple(_SPECS)
NAN_TEXEL = (3, 5)
DIRECT = ("direct",)                                 # every tile reads global memory
MIXED = ("mixed", "mixed_sizes")                     # one image direct, the other through the LDS windows
SIXTEEN_BIT = ("direct", "mixed", "mixed_sizes", "K256")
TAILS = tuple(n for n in NAMES if n[0] in "wh" or n.startswith(("out", "src")))


@functools.lru_cache(maxsize=None)
def get(name):
    return synth(name, **_SPECS[name])


@functools.lru_cache(maxsize=None)
def expected(name, dt="fp32"):
    """Per image: the CPU path on ``masks.to(dt).float()`` with fp64 ambiguity maps (inference_util.py)."""
    c = get(name)
    return iu.expected_from_cpu(c, c.masks.to(DTYPES[dt]))


@functools.lru_cache(maxsize=None)
def nan_case():
    """``nan_clean`` with one texel NaN in every query -> (case, masks, pixels the texel reaches, CPU-path results).
    Every score of such a pixel is NaN; every other pixel reads none of it and keeps the clean case's value."""
    from bm2f_amd.inference import full_resolution_logits, panoptic_counters
    c = get("nan_clean")
    masks = c.masks.clone()
    masks[:, :, NAN_TEXEL[0], NAN_TEXEL[1]] = float("nan")
    reach = full_resolution_logits(masks[0], c.padded, c.image_sizes[0], c.output_sizes[0]).isnan()
    assert reach.any() and not reach.all() and (reach == reach[0]).all()
    out = {"pred_logits": c.cls, "pred_masks": masks}
    cpu = iu.module(c)(out, c.padded, c.image_sizes, c.output_sizes)[0]
    counters = panoptic_counters(c.cls, masks, c.padded, c.image_sizes, c.output_sizes, num_classes=c.K,
                                 object_mask_threshold=c.thresholds[0])[0]
    return c, masks, reach[0].numpy(), cpu, counters.numpy().astype(np.int64)


def ramp_expected(c):
    """Per image the CPU path's sem_seg on ``cls_ramp`` (semantic head alone, logits resized before inference)."""
    m = iu.module(c, instance_on=False, panoptic_on=False, sem_seg_postprocess_before_inference=True)
    res = m({"pred_logits": c.cls_ramp, "pred_masks": c.masks}, c.padded, c.image_sizes, c.output_sizes)
    return [r["sem_seg"] for r in res]


def twin_queries(c):
    """The two queries of image 0 with identical mask (and class) logits."""
    same = [(i, j) for i in range(c.Q) for j in range(i + 1, c.Q) if torch.equal(c.masks[0, i], c.masks[0, j])]
    assert len(same) == 1
    return same[0]


def full64(c, b, masks=None):
    """The resize chain of image b in fp64: (Q, Ho, Wo)."""
    m = (c.masks if masks is None else masks)[b:b + 1].double()
    up = F.interpolate(m, size=c.padded, mode="bilinear", align_corners=False)[0]
    up = up[:, :c.image_sizes[b][0], :c.image_sizes[b][1]]
    if tuple(up.shape[-2:]) != c.output_sizes[b]:
        up = F.interpolate(up[None], size=c.output_sizes[b], mode="bilinear", align_corners=False)[0]
    return up


# ---------------------------------------------------------------------------------------------------------------------
# float32 replica of resize_device.h (bilinear_tap, axis_taps) and of semantic_kernel's tile window
# ---------------------------------------------------------------------------------------------------------------------
WIN_CAP, SEM_TILE, INSTANCE_TILE = 176, (4, 32), 1024
_f = np.float32


def bilinear_tap(dst, scale, n):
    s = _f(_f(scale * _f(_f(dst) + _f(0.5))) - _f(0.5))
    s = _f(0) if s < 0 else s
    i0 = min(int(s), n - 1)
    return i0, i0 + (1 if i0 < n - 1 else 0)


def axis_window(first, last, two, r1, in1, r2, in2):
    """Lowest and highest source index the destination range [first, last] touches (the taps are monotone)."""
    if not two:
        return bilinear_tap(first, r1, in1)[0], bilinear_tap(last, r1, in1)[1]
    return (bilinear_tap(bilinear_tap(first, r2, in2)[0], r1, in1)[0],
            bilinear_tap(bilinear_tap(last, r2, in2)[1], r1, in1)[1])


def tile_windows(c, b):
    """Source texels per query of every 4 x 32 semantic tile of image b, as the kernel computes them."""
    (h, w), (Hp, Wp), (Hc, Wc), (Ho, Wo) = c.masks.shape[-2:], c.padded, c.image_sizes[b], c.output_sizes[b]
    two = (Ho, Wo) != (Hc, Wc)
    rh1, rw1, rh2, rw2 = _f(h) / _f(Hp), _f(w) / _f(Wp), _f(Hc) / _f(Ho), _f(Wc) / _f(Wo)
    sizes = []
    for y0 in range(0, Ho, SEM_TILE[0]):
        wy0, wy1 = axis_window(y0, min(y0 + SEM_TILE[0], Ho) - 1, two, rh1, h, rh2, Hc)
        for x0 in range(0, Wo, SEM_TILE[1]):
            wx0, wx1 = axis_window(x0, min(x0 + SEM_TILE[1], Wo) - 1, two, rw1, w, rw2, Wc)
            sizes.append((wy1 - wy0 + 1) * (wx1 - wx0 + 1))
    return np.array(sizes)


def instance_tiles(c):
    return -(-max(s[0] for s in c.output_sizes) * max(s[1] for s in c.output_sizes) // INSTANCE_TILE)
