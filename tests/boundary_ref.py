"""Two independent dense oracles of the erosion behind Boundary AP, on bool arrays.  Neither shares code with
bm2f_amd; tests/test_boundary_cpu.py asserts that they agree on every case of boundary_cases.py.

The definition (mask_to_boundary of the boundary-iou-api): cv2.erode with a 3 x 3 kernel of ones, d iterations, on the
mask padded by a ring of zeros; boundary = mask & ~eroded."""
import numpy as np
from scipy import ndimage


def erode_scipy(mask, d):
    """Oracle (a): d iterations of the 3 x 3 erosion with everything outside the image zero."""
    mask = np.asarray(mask, dtype=bool)
    return ndimage.binary_erosion(mask, structure=np.ones((3, 3), dtype=bool), iterations=int(d), border_value=0)


def erode_window(mask, d):
    """Oracle (b): the minimum over the (2d + 1) x (2d + 1) window centred on the pixel, zeros outside the image."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    d = int(d)
    pad = np.zeros((H + 2 * d, W + 2 * d), dtype=bool)
    pad[d:d + H, d:d + W] = mask
    rows = np.ones((H, W + 2 * d), dtype=bool)
    for k in range(2 * d + 1):
        rows &= pad[k:k + H]
    out = np.ones((H, W), dtype=bool)
    for k in range(2 * d + 1):
        out &= rows[:, k:k + W]
    return out


def boundary(mask, d, erode=erode_scipy):
    mask = np.asarray(mask, dtype=bool)
    return mask & ~erode(mask, d)


def dilation(H, W, ratio=0.02):
    """max(1, int(round(ratio * sqrt(H^2 + W^2)))) in float64 with Python's round."""
    return max(1, int(round(ratio * np.sqrt(float(H) * H + float(W) * W))))


def iou(inter, area_d, area_g, crowd):
    union = area_d if crowd else area_d + area_g - inter
    return inter / union if union > 0 else 0.0


def boundary_iou(dt, gt, d, crowd=False):
    """min(mask IoU, boundary IoU) of two dense masks, both with COCO's crowd rule."""
    dt, gt = np.asarray(dt, dtype=bool), np.asarray(gt, dtype=bool)
    bd, bg = boundary(dt, d), boundary(gt, d)
    return min(iou(int((dt & gt).sum()), int(dt.sum()), int(gt.sum()), crowd),
               iou(int((bd & bg).sum()), int(bd.sum()), int(bg.sum()), crowd))
