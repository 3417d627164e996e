"""Inputs shared by tests/test_polygon_cpu.py and tests/test_polygon_gpu.py: the named edge cases of the polygon
rasteriser and a COCO evaluation whose ground truth is partly polygons.  The expected values always come from
tests/poly_ref.py."""
import copy

import numpy as np
import torch

import poly_ref
from bm2f_amd import rle_encode
from coco_eval_cases import load_fixture

EDGE_WIDTHS = (1, 31, 32, 33, 64, 65, 257)
EDGE_HEIGHTS = (1, 2, 37)


def edge_polygons(H, W, seed):
    """-> {name: polygon} for one image size."""
    rng = np.random.default_rng(seed)
    c = min(W - 1, 3)                                                 # a column the steep edge crosses
    out = {
        "outside_right": [W + 2, 1, W + 6, 1, W + 6, H + 3, W + 2, H + 3],
        "outside_negative": [-5, -5, -1, -5, -1, -1.5],
        # its lower edge lies below the image: the rows clamp to H in every column, the last one gives p = H * W
        "clamped_to_h": [0.0, H / 2, W, H / 2, W, H + 3, 0, H + 3],
        "clamped_to_h_middle": [W / 3, 0.2, W / 3 + 1.5, 0.2, W / 3 + 1.5, H + 7.3, W / 3, H + 7.3],
        # a repeated vertex (a zero-length edge) and purely vertical edges
        "vertical_and_zero_length": [0.4, 0.4, 0.4, 0.4, 0.4, H - 0.4, W * 0.7, H - 0.4, W * 0.7, 0.4],
        # a steep edge of dy = 5 H and dx = 1 fifth that crosses u = 5 c + 2
        "steep_bisection": [c + 0.4, 0, c + 0.6, H, c + 3, H / 2],
        "steep_bisection_down": [c + 0.6, 0, c + 0.4, H, c - 2, H / 2],
        "everything": [-3, -3, W + 3, -3, W + 3, H + 3, -3, H + 3],
    }
    for i in range(3):                                                # integer and half-integer ties
        k = int(rng.integers(3, 8))
        x = rng.integers(-2, 2 * W + 4, k) / 2.0
        y = rng.integers(-2, 2 * H + 4, k) / 2.0
        if i == 0:
            x, y = np.floor(x), np.floor(y)
        out[f"ties_{i}"] = np.stack((x, y), 1).reshape(-1).tolist()
    return out


def edge_cases():
    """-> [(name, polygon, H, W)] over EDGE_HEIGHTS x EDGE_WIDTHS."""
    out = []
    for i, H in enumerate(EDGE_HEIGHTS):
        for j, W in enumerate(EDGE_WIDTHS):
            for name, poly in edge_polygons(H, W, 100 * i + j).items():
                out.append((f"{name}@{H}x{W}", [float(v) for v in poly], H, W))
    return out


def many_parts(H, W, parts=20, seed=5):
    """An annotation of ``parts`` overlapping quadrilaterals around the image centre."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(parts):
        cx, cy = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H)
        r = rng.uniform(0.15, 0.4) * min(H, W) + 1
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))
        out.append(np.stack((cx + r * np.cos(ang), cy + r * np.sin(ang)), 1).reshape(-1).tolist())
    return out


def pack(mask):
    """(H, W) bool numpy -> (H, ceil(W / 32)) int32 numpy, written out bit by bit."""
    H, W = mask.shape
    out = np.zeros((H, (W + 31) // 32), dtype=np.int64)
    for y, x in zip(*np.nonzero(mask)):
        out[y, x // 32] |= 1 << (x % 32)
    return (out & 0xffffffff).astype(np.uint32).view(np.int32)


def polygon_ground_truth():
    """The COCO fixture with the segmentation of every second non-crowd annotation replaced by polygons made from its
    box (an octagon with fractional corners; every other one gets a second, overlapping part), the crowd RLEs kept.
    -> (gt with polygons, the same gt with the oracle's RLE of those polygons, results)."""
    gt, results, _ = load_fixture()
    sizes = {im["id"]: (im["height"], im["width"]) for im in gt["images"]}
    poly_gt, rle_gt = copy.deepcopy(gt), copy.deepcopy(gt)
    n = 0
    for a_poly, a_rle in zip(poly_gt["annotations"], rle_gt["annotations"]):
        if a_poly["iscrowd"]:
            continue
        n += 1
        if n % 2:
            continue
        x, y, w, h = a_poly["bbox"]
        k = 0.29
        parts = [[x + k * w, y - 0.3, x + w - k * w, y, x + w + 0.4, y + k * h, x + w, y + h - k * h,
                  x + w - k * w, y + h + 0.25, x + k * w, y + h, x, y + h - k * h, x - 0.6, y + k * h]]
        if n % 4 == 0:
            parts.append([x + 0.5 * w, y + 0.5 * h, x + 1.2 * w, y + 0.6 * h, x + 0.7 * w, y + 1.3 * h])
        H, W = sizes[a_poly["image_id"]]
        a_poly["segmentation"] = parts
        a_rle["segmentation"] = rle_encode(torch.from_numpy(poly_ref.annotation_mask(parts, H, W))[None])[0]
    assert n >= 8 and any(a["iscrowd"] for a in poly_gt["annotations"])
    return poly_gt, rle_gt, results
