"""The oracle of the polygon tests: a scalar, loop-by-loop transcription of the definition of the COCO polygon
rasteriser (rules 1-5 of DESIGN.md §3).  It walks every point of every edge, one after the other, collects the
crossings and sorts them.  It shares nothing with bm2f_amd.polygon: no helper, no closed form, no binary search.
Python floats are IEEE doubles, every operation is rounded on its own, and ``int()`` truncates toward zero."""
import numpy as np


def boundary_points(poly):
    """Rules 1 and 2: the points (u, v) of all edges, edge after edge, each edge from its first vertex to its second."""
    k = len(poly) // 2
    X = [int(5 * float(poly[2 * j]) + 0.5) for j in range(k)]
    Y = [int(5 * float(poly[2 * j + 1]) + 0.5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    pts = []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx >= dy:
            if dx == 0:
                pts.append((xs, ys))                                  # a single point: it can yield nothing
                continue
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flip else d
                pts.append((t + xs, int(ys + s * t + 0.5)))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                pts.append((int(xs + s * t + 0.5), t + ys))
    return pts


def crossings(poly, h, w):
    """Rule 3 -> the sorted positions, the sentinel h * w included."""
    pts = boundary_points(poly)
    out = []
    for j in range(1, len(pts)):
        (u0, v0), (u1, v1) = pts[j - 1], pts[j]
        if u0 == u1:
            continue
        u, v = min(u0, u1), min(v0, v1)
        if (u - 2) % 5 != 0:
            continue
        c = (u - 2) // 5
        if c < 0 or c > w - 1:
            continue
        y = (v + 0.5) / 5 - 0.5
        y = 0.0 if y < 0 else float(h) if y > h else y
        row = int(np.ceil(y))
        out.append(c * h + row)
    out.append(h * w)
    return sorted(out)


def polygon_mask(poly, h, w):
    """Rule 4 -> (h, w) bool."""
    flips = np.zeros(h * w + 1, dtype=np.int64)
    for p in crossings(poly, h, w):
        flips[p] += 1
    return ((np.cumsum(flips[:h * w]) & 1) == 1).reshape(w, h).T


def annotation_mask(polys, h, w):
    """Rule 5 -> (h, w) bool."""
    out = np.zeros((h, w), dtype=bool)
    for poly in polys:
        out |= polygon_mask(poly, h, w)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the seeded sweep shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def sweep(n=2000, seed=20261020):
    """-> [(polygon as a flat list, h, w)]: 3-12 vertices, h, w in [1, 70], coordinates on integers, on halves or
    arbitrary, up to 30 % outside on every side (so negative too), a repeated vertex in every fifth polygon."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        k = int(rng.integers(3, 13))
        x = rng.uniform(-0.3 * w, 1.3 * w, k)
        y = rng.uniform(-0.3 * h, 1.3 * h, k)
        mode = i % 3
        if mode == 0:
            x, y = np.round(x), np.round(y)
        elif mode == 1:
            x, y = np.round(2 * x) / 2, np.round(2 * y) / 2
        if i % 5 == 0:
            j = int(rng.integers(0, k))
            x[(j + 1) % k], y[(j + 1) % k] = x[j], y[j]
        out.append((np.stack((x, y), 1).reshape(-1).tolist(), h, w))
    return out


_cache = {}


def sweep_reference():
    """The sweep with the oracle's positions and masks, computed once per session and never modified."""
    if "sweep" not in _cache:
        cases = sweep()
        _cache["sweep"] = (cases, [crossings(p, h, w) for p, h, w in cases],
                           [polygon_mask(p, h, w) for p, h, w in cases])
    return _cache["sweep"]
