"""Generate the video AP fixtures (ytvis_eval_gt.json, ytvis_eval_results.json, ytvis_eval_expected.npz) by running
the reference's ``YTVOS`` and ``YTVOSeval`` on a seeded synthetic dataset (nothing from the reference tree is copied).

    python tests/golden/gen_ytvis_eval_golden.py --ref /path/to/reference

The reference modules import ``matplotlib`` and ``pycocotools.mask``; neither is a dependency here, so stand-ins are
installed before the import.  The ``pycocotools.mask`` stand-in (``area``, ``merge``, ``frPyObjects`` for
uncompressed RLE, ``toBbox``, ``decode``, ``encode``) is written below from dense numpy masks with its own loop
reader and writer of the RLE strings.  So the matching, accumulation and summary in the fixtures are the reference's,
and the IoU in them comes from a dense definition that shares no code with bm2f_amd.

Frames are 300 x 420 so that the small, medium and large area ranges all occur.  The branches the data must reach
are asserted at the end (``check_coverage``): the run fails rather than writing fixtures that miss one.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ytvis_eval_cases import CONFIGS, EXPECTED_NPZ, GT_JSON, RESULTS_JSON, flatten  # noqa: E402

H, W = 300, 420


# -------------------------------------------------------------------------------------------------------------------
# a dense stand-in for pycocotools.mask
# -------------------------------------------------------------------------------------------------------------------
def _read(s):
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p, k = p + 1, k + 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def _write(counts):
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
    return "".join(out)


def _dense(rle):
    if "_dense" in rle:
        return rle["_dense"]
    h, w = rle["size"]
    counts = rle["counts"] if isinstance(rle["counts"], list) else _read(rle["counts"])
    assert sum(counts) == h * w and min(counts) >= 0
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    return flat.reshape(w, h).T


def _counts(mask):
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.flatnonzero(np.diff(np.concatenate(([False], flat)).astype(np.int8)) != 0)
    return np.diff(np.concatenate(([0], edges, [flat.size]))).tolist()


def encode_mask(mask):
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": _write(_counts(mask))}


def make_mask_module():
    m = types.ModuleType("pycocotools.mask")

    def one_or_many(fn):
        return lambda r, *a: [fn(x, *a) for x in r] if isinstance(r, list) else fn(r, *a)

    def merge(rles, intersect=False):
        planes = [_dense(r) for r in rles]
        out = planes[0].copy()
        for q in planes[1:]:
            out = out & q if intersect else out | q
        return {"size": list(out.shape), "_dense": out}

    def bbox(r):
        ys, xs = np.nonzero(_dense(r))
        if ys.size == 0:
            return np.zeros(4)
        return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], dtype=np.float64)

    def from_uncompressed(obj, h, w):
        assert isinstance(obj, dict) and isinstance(obj["counts"], list), "only uncompressed RLE"
        return {"size": [h, w], "counts": _write(obj["counts"]).encode("ascii")}

    m.area = one_or_many(lambda r: np.uint32(_dense(r).sum()))
    m.merge = merge
    m.toBbox = one_or_many(bbox)
    m.decode = one_or_many(lambda r: _dense(r).astype(np.uint8))
    m.encode = lambda a: {**encode_mask(np.asarray(a) != 0), "counts": _write(_counts(np.asarray(a) != 0)).encode()}
    m.frPyObjects = from_uncompressed
    m.iou = None
    return m


def import_reference(ref_root):
    pkg = types.ModuleType("pycocotools")
    pkg.mask = make_mask_module()
    sys.modules["pycocotools"] = pkg
    sys.modules["pycocotools.mask"] = pkg.mask
    for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.collections", "matplotlib.patches"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib.collections"].PatchCollection = object
    sys.modules["matplotlib.patches"].Polygon = object
    api = os.path.join(ref_root, "mask2former_video", "data_video", "datasets", "ytvis_api")
    sys.path.insert(0, api)
    import ytvos
    import ytvoseval
    return ytvos, ytvoseval


# -------------------------------------------------------------------------------------------------------------------
# the dataset
# -------------------------------------------------------------------------------------------------------------------
def rect(y0, y1, x0, x1):
    m = np.zeros((H, W), dtype=bool)
    m[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = True
    return m


def ellipse(cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


class Builder:
    def __init__(self):
        self.videos, self.anns, self.results = [], [], []

    def video(self, vid, length):
        self.videos.append({"id": vid, "height": H, "width": W, "length": length,
                            "file_names": [f"v{vid}/{t:05d}.jpg" for t in range(length)]})

    def gt(self, vid, cat, frames, iscrowd=0, uncompressed=False):
        """frames: one mask or None per frame."""
        segs, areas = [], []
        for m in frames:
            if m is None:
                segs.append(None)
                areas.append(None)
            else:
                segs.append({"size": [H, W], "counts": _counts(m)} if uncompressed else encode_mask(m))
                areas.append(int(m.sum()))
        self.anns.append({"id": len(self.anns) + 1, "video_id": vid, "category_id": cat, "iscrowd": iscrowd,
                          "segmentations": segs, "areas": areas, "bboxes": [None] * len(frames)})

    def det(self, vid, cat, score, frames):
        self.results.append({"video_id": vid, "score": float(score), "category_id": cat,
                             "segmentations": [None if m is None else encode_mask(m) for m in frames]})


def build_dataset():
    b = Builder()
    rng = np.random.RandomState(7)
    empty = np.zeros((H, W), dtype=bool)

    # video 1, category 1: a regular small ground truth and a medium crowd that two detections match; the detection
    # on the regular one then meets the crowd (the break); a far detection stays unmatched
    b.video(1, 2)
    small = [rect(20, 80, 30, 90), rect(24, 84, 34, 94)]
    crowd = [rect(100, 260, 150, 330), rect(100, 260, 154, 334)]
    b.gt(1, 1, small)
    b.gt(1, 1, crowd, iscrowd=1, uncompressed=True)
    b.det(1, 1, 0.9, [rect(22, 80, 30, 88), rect(24, 84, 36, 94)])
    b.det(1, 1, 0.8, [rect(104, 260, 150, 326), rect(100, 256, 154, 334)])
    b.det(1, 1, 0.8, [rect(100, 252, 156, 330), rect(108, 260, 154, 330)])        # equal score in one video
    b.det(1, 1, 0.3, [rect(270, 298, 380, 418), rect(270, 298, 380, 418)])
    # video 1, category 2: a large ground truth seen in the first frame only, a detection missing the second frame
    large = rect(10, 290, 60, 330)
    b.gt(1, 2, [large, None])
    b.det(1, 2, 0.7, [rect(14, 290, 60, 326), None])
    b.det(1, 2, 0.6, [rect(10, 150, 60, 330), empty])                             # a frame of area 0

    # video 2: category 2 has ground truth and no detection, category 3 detections and no ground truth
    b.video(2, 2)
    b.gt(2, 2, [ellipse(150, 200, 60, 90), ellipse(152, 204, 60, 90)])
    b.det(2, 3, 0.8, [ellipse(80, 100, 30, 40), ellipse(80, 104, 30, 40)])        
    b.det(2, 3, 0.2, [rect(200, 290, 300, 400), rect(200, 290, 300, 400)])

    # video 3, category 1: seven detections, more than the reduced maxDets[-1] = 5, on three ground truths
    b.video(3, 3)
    objs = [(40, 60, 30, 40), (150, 200, 70, 110), (230, 340, 50, 60)]
    for cy, cx, ry, rx in objs:
        b.gt(3, 1, [ellipse(cy + 2 * t, cx + 3 * t, ry, rx) for t in range(3)], uncompressed=cx == 200)
    for n in range(7):                                                # scores 0.9, 0.8, ...: equal to video 1's
        cy, cx, ry, rx = objs[n % 3]
        dy, dx = rng.randint(-12, 13, size=2)
        b.det(3, 1, round(0.9 - 0.1 * n, 2), [ellipse(cy + dy + 2 * t, cx + dx + 3 * t, ry + n, rx - n)
                                              for t in range(3)])

    # video 4, category 2: intersection 1 of union 2, IoU exactly 0.5; category 3: a pair with union 0
    b.video(4, 2)
    two = empty.copy()
    two[5, 7] = two[6, 7] = True
    one = empty.copy()
    one[5, 7] = True
    b.gt(4, 2, [two, None])
    b.det(4, 2, 0.5, [one, None])
    b.gt(4, 3, [None, None])
    b.det(4, 3, 0.4, [empty, empty])

    # videos 5-7: jittered copies of random objects in categories 1-3, with misses and false positives
    for vid in (5, 6, 7):
        b.video(vid, 2)
        for _ in range(rng.randint(2, 5)):
            cat = int(rng.randint(1, 4))
            ry, rx = rng.randint(15, 140), rng.randint(20, 190)
            cy, cx = rng.randint(ry, H - ry), rng.randint(rx, W - rx)
            b.gt(vid, cat, [ellipse(cy, cx, ry, rx), ellipse(cy + 3, cx - 4, ry, rx)], uncompressed=bool(rng.rand() < 0.3))
            for _ in range(rng.randint(0, 3)):
                jy, jx = rng.randint(-ry // 3 - 1, ry // 3 + 2), rng.randint(-rx // 3 - 1, rx // 3 + 2)
                s = round(float(rng.rand()), 3)
                wrong = int(rng.randint(1, 4)) if rng.rand() < 0.2 else cat
                b.det(vid, wrong, s, [ellipse(cy + jy, cx + jx, ry, rx), ellipse(cy + jy + 3, cx + jx - 4, ry + 2, rx)])
    categories = [{"id": i, "name": n, "supercategory": "object"}
                  for i, n in enumerate(("person", "dog", "car", "kite"), start=1)]     # category 4 stays empty
    return {"videos": b.videos, "categories": categories, "annotations": b.anns,
            "info": {"description": "synthetic"}}, b.results


# -------------------------------------------------------------------------------------------------------------------
# run the reference
# -------------------------------------------------------------------------------------------------------------------
def run_reference(mods, gt_path, results, max_dets, trace_lines):
    ytvos, ytvoseval = mods
    code = ytvoseval.YTVOSeval.evaluateVid.__code__
    seen = set()

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(frame, event, arg):
            if event == "line" and frame.f_lineno in trace_lines:
                seen.add(frame.f_lineno)
            return local
        return local

    with contextlib.redirect_stdout(io.StringIO()):
        gt = ytvos.YTVOS(gt_path)
        dt = gt.loadRes(json.loads(json.dumps(results)))
        ev = ytvoseval.YTVOSeval(gt, dt)
        ev.params.maxDets = list(max_dets)
        sys.settrace(tracer)
        try:
            ev.evaluate()
        finally:
            sys.settrace(None)
        ev.accumulate()
        ev.summarize()
    return ev, seen


def check_coverage(gt, results, evals, seen, break_line):
    """Every branch the issue lists is reached by the committed data."""
    ev = evals["default"]
    red = evals["reduced"]
    imgs = [e for e in ev.evalImgs if e is not None]
    ann = {a["id"]: a for a in gt["annotations"]}
    crowd_ids = {a["id"] for a in gt["annotations"] if a["iscrowd"]}
    thr0 = 0
    assert any(sum(1 for g in e["dtMatches"][thr0] if g in crowd_ids) >= 2 for e in imgs), "crowd matched twice"
    assert any(e["gtIgnore"][i] and gid not in crowd_ids for e in imgs for i, gid in enumerate(e["gtIds"])), \
        "ground truth ignored by area range"
    assert any(e["gtIgnore"][i] and gid in crowd_ids for e in imgs for i, gid in enumerate(e["gtIds"])), \
        "ground truth ignored as crowd"
    assert any(((e["dtMatches"] == 0) & e["dtIgnore"]).any() for e in imgs), "unmatched detection outside the range"
    assert any(((e["dtMatches"] > 0) & e["dtIgnore"]).any() for e in imgs), "detection matched to an ignored gt"
    assert break_line in seen, "the break on ignore never fired"
    assert any(s is None for r in results for s in r["segmentations"]), "detection with a missing frame"
    assert any(s is None for a in gt["annotations"] for s in a["segmentations"]), "ground truth with a missing frame"
    assert any(s is not None and _dense(s).sum() == 0 for r in results for s in r["segmentations"]), "area-0 frame"
    gt_keys = {(a["video_id"], a["category_id"]) for a in gt["annotations"]}
    dt_keys = {(r["video_id"], r["category_id"]) for r in results}
    assert gt_keys - dt_keys and dt_keys - gt_keys, "a pair with only ground truth and one with only detections"
    used = {c for _, c in gt_keys | dt_keys}
    absent = [k for k, c in enumerate(sorted(x["id"] for x in gt["categories"])) if c not in used]
    assert absent and (ev.eval["precision"][:, :, absent] == -1).all(), "a category absent everywhere"
    per_key = {}
    for r in results:
        per_key.setdefault((r["video_id"], r["category_id"]), []).append(r["score"])
    assert any(len(s) != len(set(s)) for s in per_key.values()), "equal scores in one video"
    by_cat = {}
    for (v, c), s in per_key.items():
        for x in s:
            by_cat.setdefault((c, x), set()).add(v)
    assert any(len(v) > 1 for v in by_cat.values()), "equal scores across videos"
    limit = CONFIGS["reduced"][-1]
    assert any(len(s) > limit for s in per_key.values()), "more detections than the reduced maxDets[-1]"
    assert all(len(e["dtIds"]) <= limit for e in red.evalImgs if e is not None)
    halves = [(k, v) for k, v in ev.ious.items() if len(v) and (np.asarray(v) == 0.5).any()]
    assert halves, "an IoU exactly at a threshold"
    whole = [e for e in imgs if e["aRng"][0] == 0 and e["aRng"][1] > 1e9
             and any((e["video_id"], e["category_id"]) == k and np.asarray(v).shape == (1, 1) for k, v in halves)]
    assert whole and whole[0]["dtMatches"][0].any() and not whole[0]["dtMatches"][1].any(), \
        "IoU 0.5 matches at 0.5 only"
    # union 0: a ground truth without frames against a detection without pixels
    zero = [a for a in gt["annotations"] if not any(a["segmentations"])]
    assert zero and any((r["video_id"], r["category_id"]) == (zero[0]["video_id"], zero[0]["category_id"])
                        and all(s is not None and _dense(s).sum() == 0 for s in r["segmentations"])
                        for r in results), "a pair with union 0"
    for name in ("small", "medium", "large"):
        i = ev.params.areaRngLbl.index(name)
        assert (ev.eval["recall"][:, :, i, -1] > -1).any(), f"no ground truth in the {name} range"
    assert ann and ev.stats[0] > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    mods = import_reference(a.ref)
    gt, results = build_dataset()
    with open(GT_JSON, "w") as f:
        json.dump(gt, f, separators=(",", ":"))
    with open(RESULTS_JSON, "w") as f:
        json.dump(results, f, separators=(",", ":"))
    import inspect
    src, first = inspect.getsourcelines(mods[1].YTVOSeval.evaluateVid)
    break_line = first + next(i for i, line in enumerate(src) if line.strip() == "break")
    evals, arrays, seen = {}, {}, set()
    for name, max_dets in CONFIGS.items():
        ev, s = run_reference(mods, GT_JSON, results, max_dets, {break_line})
        seen |= s
        evals[name] = ev
        flat = flatten(ev.ious, ev.evalImgs, ev.eval["precision"], ev.eval["recall"], ev.eval["scores"], ev.stats,
                       len(ev.params.iouThrs))
        arrays.update({f"{name}/{k}": v for k, v in flat.items()})
    check_coverage(gt, results, evals, seen, break_line)
    np.savez_compressed(EXPECTED_NPZ, **arrays)
    for p in (GT_JSON, RESULTS_JSON, EXPECTED_NPZ):
        print(p, os.path.getsize(p), "bytes")
    print("stats", {k: np.round(v.stats, 4).tolist() for k, v in evals.items()})


if __name__ == "__main__":
    main()
