"""Cases of the input-view tests (test_image_views_cpu.py, test_image_views_gpu.py) and of the generator of
tests/golden/image_views.npz.  Inputs are regenerated from seeds; the fixture holds only what Pillow made of them:
the SHA-256 of a case's canvas (equality with a digest is still equality; test_image_views_cpu.py also compares
with Pillow itself, element by element), and the whole canvas where a test assembles a batch from it.

The geometry after the resize (crop window, mirror, canvas) is restated here in plain numpy, apart from the package."""
import hashlib
import zlib

import numpy as np

MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]     # the Mask2Former configs' PIXEL_MEAN / PIXEL_STD

# (H, W) -> (h, w): up, non-integer down, one pass skipped (twice), ksize 31, 9x9 up, degenerate axes, and a pair that
# crosses the kernel's 64-column and 16-row tiles in both axes with remainders
PAIRS = [((37, 53), (64, 91)), ((37, 53), (19, 23)), ((64, 48), (64, 100)), ((50, 70), (13, 70)), ((101, 77), (7, 5)),
         ((9, 9), (64, 64)), ((1, 5), (3, 7)), ((5, 1), (7, 3)), ((40, 40), (1, 1)), ((37, 53), (70, 131))]
LABEL_PAIRS = PAIRS + [((200, 3), (50, 9))]


def seed_of(name):
    return zlib.crc32(name.encode())


def content(kind, shape, name):
    if kind == "rand":
        return np.random.default_rng(seed_of(name)).integers(0, 256, shape, dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.indices(shape[:2])
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], shape).copy()
    return np.full(shape, {"255": 255, "0": 0}[kind], dtype=np.uint8)


def _case(name, src, size, kind="rand", **kw):
    return dict(name=name, src=src, size=size, kind=kind, crop=kw.get("crop"), canvas=kw.get("canvas"),
                flip_in=kw.get("flip_in", False), flip_out=kw.get("flip_out", False), fill=kw.get("fill", 0))


def _image_cases():
    cases = [_case(f"pair{i}", s, d) for i, (s, d) in enumerate(PAIRS)]
    for i in (0, 1, 4):                                     # clip8 (all 255), zeros, the sharpest edges
        cases += [_case(f"pair{i}_{k}", *PAIRS[i], kind=k) for k in ("255", "0", "checker")]
    for tag, s, d in (("small", (37, 53), (19, 23)), ("tiles", (37, 53), (35, 70))):
        cases += [_case(f"flip_in_{tag}", s, d, flip_in=True), _case(f"flip_out_{tag}", s, d, flip_out=True),
                  _case(f"flip_both_{tag}", s, d, flip_in=True, flip_out=True)]
    s, d = (37, 53), (35, 70)
    cases += [_case("crop_mid_tile", s, d, crop=(17, 30, 18, 40)),
              _case("crop_mid_tile_flip", s, d, crop=(17, 30, 18, 40), flip_out=True),
              _case("crop_one_pixel", s, d, crop=(34, 69, 1, 1)),
              _case("crop_past_image", s, d, crop=(25, 50, 20, 30), fill=128),
              _case("crop_past_image_flips", s, d, crop=(25, 50, 20, 30), fill=128, flip_in=True, flip_out=True),
              _case("crop_before_image", s, d, crop=(-3, -2, 10, 12), fill=128),
              _case("canvas_larger", s, d, crop=(5, 7, 20, 30), canvas=(33, 75), fill=128),
              _case("canvas_smaller", s, d, canvas=(20, 66), fill=7)]
    return cases


IMAGE_CASES = _image_cases()
IMAGE_BY_NAME = {c["name"]: c for c in IMAGE_CASES}


def image_source(case):
    return content(case["kind"], (*case["src"], 3), case["name"])


LABEL_DTYPES = {"uint8": (np.uint8, 0, 256), "int16": (np.int16, -7, 30000), "int32": (np.int32, -9, 1 << 30)}


def _label_cases():
    cases = []
    for dt in LABEL_DTYPES:
        for i, (s, d) in enumerate(LABEL_PAIRS):
            cases.append(dict(_case(f"lab_{dt}_pair{i}", s, d), dtype=dt, planes=1, seg_pad=255 if dt == "uint8" else 0))
        for i in (0, 1, 10):
            cases.append(dict(_case(f"lab_{dt}_p3_pair{i}", *LABEL_PAIRS[i]), dtype=dt, planes=3, seg_pad=0))
        s, d = (37, 53), (35, 70)
        for tag, kw in (("flip_in", dict(flip_in=True)), ("flip_both", dict(flip_in=True, flip_out=True)),
                        ("crop_past", dict(crop=(25, 50, 20, 30), flip_out=True)),
                        ("canvas", dict(crop=(5, 7, 20, 30), canvas=(33, 75)))):
            cases.append(dict(_case(f"lab_{dt}_{tag}", s, d, **kw), dtype=dt, planes=3 if tag == "canvas" else 1,
                              seg_pad=255 if tag != "canvas" else 0))
    return cases


LABEL_CASES = _label_cases()


def label_source(case):
    dt, lo, hi = LABEL_DTYPES[case["dtype"]]
    rng = np.random.default_rng(seed_of(case["name"]))
    return rng.integers(lo, hi, (case["planes"], *case["src"])).astype(dt)


def place(resized, case, fill):
    """Crop window, mirror and canvas on a channels-first (C, h, w) resized array, element by plain slicing."""
    rh, rw = resized.shape[1:]
    y0, x0, ch, cw = case["crop"] or (0, 0, rh, rw)
    Hc, Wc = case["canvas"] or (ch, cw)
    win = np.full((resized.shape[0], ch, cw), fill, dtype=resized.dtype)
    for y in range(ch):
        if 0 <= y0 + y < rh:
            xa, xb = max(x0, 0), min(x0 + cw, rw)
            if xb > xa:
                win[:, y, xa - x0:xb - x0] = resized[:, y0 + y, xa:xb]
    if case["flip_out"]:
        win = win[:, :, ::-1]
    out = np.full((resized.shape[0], Hc, Wc), fill, dtype=resized.dtype)
    h, w = min(ch, Hc), min(cw, Wc)
    out[:, :h, :w] = win[:, :h, :w]
    return out


def pil_image(case, src=None):
    """What the reference's host route makes of an image case: Pillow's resize, then the geometry."""
    from PIL import Image
    src = image_source(case) if src is None else src
    src = np.ascontiguousarray(src[:, ::-1]) if case["flip_in"] else src
    h, w = case["size"]
    r = np.asarray(Image.fromarray(src).resize((w, h), Image.BILINEAR))
    return place(np.moveaxis(r, 2, 0), case, case["fill"])


def pil_label(case, src=None):
    """Pillow's NEAREST per plane in mode "I" (32-bit), which holds all three element types; cast back."""
    from PIL import Image
    src = label_source(case) if src is None else src
    h, w = case["size"]
    planes = []
    for p in src:
        p = np.ascontiguousarray(p[:, ::-1] if case["flip_in"] else p).astype(np.int32)
        planes.append(np.asarray(Image.fromarray(p, mode="I").resize((w, h), Image.NEAREST)).astype(src.dtype))
    return place(np.stack(planes), case, case["seg_pad"])


# the ragged batch: 4 views of 3 sources, source 2 a strided crop view (rows 5:30, columns 11:51) of a 40 x 60 tensor
RAGGED_SOURCES = [(20, 30), (33, 17), (25, 40)]
RAGGED_BIG, RAGGED_WINDOW = (40, 60), (5, 11)
RAGGED_VIEWS = [dict(_case("ragged0", RAGGED_SOURCES[0], (30, 40)), source=0),
                dict(_case("ragged1", RAGGED_SOURCES[1], (16, 24), flip_out=True), source=1),
                dict(_case("ragged2", RAGGED_SOURCES[2], (20, 70), crop=(2, 3, 18, 66), canvas=(19, 67), fill=128),
                     source=2),
                dict(_case("ragged3", RAGGED_SOURCES[2], (40, 20), flip_in=True), source=2)]


def ragged_sources():
    big = content("rand", (*RAGGED_BIG, 3), "ragged_big")
    y, x = RAGGED_WINDOW
    h, w = RAGGED_SOURCES[2]
    return [content("rand", (*RAGGED_SOURCES[0], 3), "ragged_s0"), content("rand", (*RAGGED_SOURCES[1], 3), "ragged_s1"),
            big[y:y + h, x:x + w]], big


# DeviceTTAMapper and preprocess_test_images
TTA = dict(min_sizes=(16, 24), max_size=40, shape=(20, 30))
PREP = dict(min_size=24, max_size=40, shapes=[(20, 30), (31, 18)], size_divisibility=32)


def tta_image():
    return content("rand", (*TTA["shape"], 3), "tta")


def prep_images():
    return [content("rand", (*s, 3), f"prep{i}") for i, s in enumerate(PREP["shapes"])]


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def record(store, name, a, full=False):
    """Into the generator's dict: whole under ``name``, or as one row of the "names" / "shapes" / "sha" tables."""
    a = np.ascontiguousarray(a)
    if full:
        store[name] = a
    else:
        store.setdefault("_rows", []).append((name, a.shape, digest(a)))


def finish(store):
    rows = store.pop("_rows")
    store["names"] = np.array([r[0] for r in rows], dtype="S40")
    store["shapes"] = np.array([r[1] for r in rows], dtype=np.int32)
    store["sha"] = np.stack([r[2] for r in rows])
    return store


def matches(fixture, name, got):
    """got equals what the fixture recorded under ``name``: its shape and its bytes (whole or by digest)."""
    got = np.ascontiguousarray(got)
    if name in fixture:
        return fixture[name].dtype == got.dtype and np.array_equal(fixture[name], got)
    (i,) = np.nonzero(fixture["names"] == name.encode())[0]
    return tuple(fixture["shapes"][i]) == got.shape and np.array_equal(fixture["sha"][i], digest(got))
