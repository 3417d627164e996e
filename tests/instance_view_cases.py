"""The cases of the instance-view tests (CPU and GPU) and of tests/golden/gen_instance_views_golden.py.

A case is a source size, a view and the six masks below; every case is the smallest shape at which its path can go
wrong.  The masks are regenerated from seeds, so the golden file stores only Pillow's outputs (bit-packed)."""
import numpy as np

from bm2f_amd.image_views import View

KINDS = ("empty", "full", "first", "last", "noise", "blob")

# name, source (H, W), view.  Output widths 1, 31, 32, 33, 63, 65 and 95; source widths 33 and 70 (2 and 3 words with
# a tail); an up-scale and a down-scale per axis; both flips; crops past the image; a canvas beyond the crop
CASES = [
    dict(name="up_w65", hw=(40, 33), view=View(size=(80, 65))),                       # 80 rows: three row bands
    dict(name="down_w31", hw=(40, 70), view=View(size=(20, 31))),
    dict(name="mixed_crop_w32", hw=(40, 33), view=View(size=(20, 66), crop=(3, 2, 17, 32))),
    dict(name="flip_in_w33", hw=(40, 70), view=View(size=(60, 35), crop=(0, 1, 50, 33), flip_in=True)),
    dict(name="flip_out_w1", hw=(40, 33), view=View(size=(40, 33), crop=(5, 4, 30, 1), flip_out=True)),
    dict(name="both_flips_past_w63", hw=(40, 70),
         view=View(size=(50, 90), crop=(10, 40, 60, 63), flip_in=True, flip_out=True)),  # past right and bottom
    dict(name="canvas_w95", hw=(40, 33), view=View(size=(45, 50), canvas=(64, 95))),
    dict(name="before_image_w50", hw=(40, 70), view=View(size=(30, 40), crop=(-3, -2, 40, 50), flip_out=True)),
    dict(name="canvas_cuts_crop", hw=(40, 33), view=View(size=(50, 41), crop=(2, 3, 40, 36), canvas=(32, 32))),
]


def case_masks(hw, kinds=KINDS, seed=0):
    """(len(kinds), H, W) uint8 masks of 0 / 1."""
    H, W = hw
    rng = np.random.default_rng(1000 * H + W + seed)
    out = np.zeros((len(kinds), H, W), dtype=np.uint8)
    for i, k in enumerate(kinds):
        if k == "full":
            out[i] = 1
        elif k == "first":
            out[i, 0, 0] = 1
        elif k == "last":
            out[i, H - 1, W - 1] = 1
        elif k == "noise":
            out[i] = rng.random((H, W)) < 0.3
        elif k == "blob":
            y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
            out[i, y0:y0 + H // 3, x0:x0 + W // 2] = 1
    return out


def pack(masks, garbage=None):
    """(M, H, W) uint8 -> (M, H, ceil(W / 32)) int32 words; ``garbage`` (a Generator) sets the tail bits at random."""
    M, H, W = masks.shape
    words = (W + 31) // 32
    pad = np.zeros((M, H, words * 32), dtype=np.uint8)
    pad[..., :W] = masks
    if garbage is not None:
        pad[..., W:] = garbage.integers(0, 2, size=(M, H, words * 32 - W))
    return np.packbits(pad, axis=-1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def unpack(words, W):
    """(..., words) int32 -> (..., W) uint8, and whether every tail bit is zero."""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :W], not bits[..., W:].any()


def ragged(mask_lists, garbage=None, gap=3):
    """Masks of several images -> (words (flat int32), offsets, sizes, view_of_mask): image i's masks name view i;
    ``gap`` padding words between planes, garbage when asked for."""
    parts, offsets, sizes, view_of, at = [], [], [], [], 0
    for v, masks in enumerate(mask_lists):
        for plane in pack(masks, garbage) if len(masks) else []:
            offsets.append(at)
            sizes.append(masks.shape[1:])
            view_of.append(v)
            filler = (np.zeros(gap, np.int32) if garbage is None
                      else garbage.integers(-2 ** 31, 2 ** 31, size=gap).astype(np.int32))
            parts += [plane.reshape(-1), filler]
            at += plane.size + gap
    words = np.concatenate(parts) if parts else np.zeros(1, np.int32)
    return (words, np.asarray(offsets, np.int64), np.asarray(sizes, np.int64).reshape(-1, 2),
            np.asarray(view_of, np.int64))


def place(resized, view):
    """numpy crop, flip and zero pad of a resized (rh, rw) mask: the view's canvas."""
    rh, rw = resized.shape
    cy0, cx0, ch, cw = view.crop if view.crop is not None else (0, 0, rh, rw)
    Hc, Wc = view.canvas if view.canvas is not None else (ch, cw)
    win = np.zeros((ch, cw), dtype=np.uint8)
    for y in range(ch):
        for x in range(cw):
            if 0 <= cy0 + y < rh and 0 <= cx0 + x < rw:
                win[y, x] = resized[cy0 + y, cx0 + x]
    if view.flip_out:
        win = win[:, ::-1]
    canvas = np.zeros((Hc, Wc), dtype=np.uint8)
    canvas[:min(ch, Hc), :min(cw, Wc)] = win[:min(ch, Hc), :min(cw, Wc)]
    return canvas


def pil_view(mask, view):
    """``transform_instance_annotations`` on a decoded mask with Pillow: flip, ``resize(NEAREST)``, crop, flip, pad."""
    from PIL import Image
    m = np.ascontiguousarray(mask[:, ::-1] if view.flip_in else mask)
    resized = np.asarray(Image.fromarray(m).resize((view.size[1], view.size[0]), Image.NEAREST))
    return place(resized, view)


def bitmask_boxes(masks):
    """``BitMasks.get_bounding_boxes`` restated literally, and ``sum``: (M, 4) float32, (M,) int32."""
    boxes = np.zeros((masks.shape[0], 4), dtype=np.float32)
    x_any, y_any = masks.any(axis=1), masks.any(axis=2)
    for idx in range(masks.shape[0]):
        x, y = np.where(x_any[idx])[0], np.where(y_any[idx])[0]
        if len(x) > 0 and len(y) > 0:
            boxes[idx] = (x[0], y[0], x[-1] + 1, y[-1] + 1)
    return boxes, masks.reshape(masks.shape[0], -1).sum(axis=1).astype(np.int32)


# the batch: images with 70, 0, 1 and 6 instances under views of different sizes, padded to a multiple of 32
BATCH = [("up_w65", ("noise",) * 70), ("down_w31", ()), ("both_flips_past_w63", ("blob",)), ("canvas_w95", KINDS)]


def batch_masks():
    by_name = {c["name"]: c for c in CASES}
    cases = [by_name[n] for n, _ in BATCH]
    lists = [np.concatenate([case_masks(c["hw"], (k,), seed=j) for j, k in enumerate(kinds)]) if kinds
             else np.zeros((0,) + c["hw"], np.uint8) for c, (_, kinds) in zip(cases, BATCH)]
    return cases, lists


def golden_store(fn):
    """{key: bit-packed outputs of ``fn(mask, view)``} for every case and the batch."""
    store = {}
    for c in CASES:
        out = np.stack([fn(m, c["view"]) for m in case_masks(c["hw"])])
        store[c["name"]] = np.packbits(out, axis=-1, bitorder="little")
    cases, lists = batch_masks()
    for i, (c, masks) in enumerate(zip(cases, lists)):
        if len(masks):
            out = np.stack([fn(m, c["view"]) for m in masks])
            store[f"batch{i}"] = np.packbits(out, axis=-1, bitorder="little")
    return store


def golden_masks(store, key, canvas):
    """The stored outputs of a case as (M, Hc, Wc) uint8."""
    return np.unpackbits(store[key], axis=-1, bitorder="little")[..., :canvas[1]]


def canvas_of(view):
    crop = view.crop if view.crop is not None else (0, 0) + tuple(view.size)
    return tuple(view.canvas) if view.canvas is not None else tuple(crop[2:])
