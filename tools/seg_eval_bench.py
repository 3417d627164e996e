"""Time the device label-pair counts (csrc/label_counts.hip under SemSegEvaluator and COCOPanopticEvaluator) against
the host route of the stack they replace: copy the label maps to the host, then ``np.bincount`` of ``(K + 1) * pred +
gt`` (detectron2's SemSegEvaluator) or ``np.unique(gt * 256^3 + pred, return_counts=True)`` (panopticapi).

    python tools/seg_eval_bench.py [--reps 5] [--device-reps 50] [--kernel-reps 100] [--out profiles/seg_eval.json]

Shapes (synthetic, seeded; both label maps start on the device, as the heads leave them):

    semantic   16 images of 512 x 683, K = 150, uint8 ground truth and int16 predictions; one shared 151 x 151 table
    panoptic   16 images of 800 x 1216, about 40 blob-like segments each over 133 categories, int32 id maps; one
               (segments + 2) x (max id + 1) table per image, id-list mode
    random     the semantic shape with per-pixel random labels: the worst case of the wave merge

Per shape: ``host_ms`` the host route (the copies to the host are part of it), ``device_ms`` one call of
``label_pair_counts_ragged`` per path ("lds", "global", and what "auto" picks), both checked for equal tables first;
``process_ms`` one whole ``process`` call of the evaluator on the device against the same call on host copies
(``process_host_ms``, which includes those copies).  Times are wall milliseconds per call (host clock, a device
synchronise before and after), the faster of two windows after a warm-up: --reps calls for the host routes (tens of
milliseconds each) and --device-reps calls for the device routes (a fraction of a millisecond each, so that a window
is some 15 ms or more).  ``kernel`` puts device events
around --kernel-reps back-to-back calls of the C entry point on buffers allocated once (the tables are not re-zeroed:
the counts run on, the work is the same): kernel time plus any gap the host leaves between enqueues, so an upper bound
on kernel time; the bytes are every label read once.  The window re-reads the same 17 MB (semantic) or 125 MB
(panoptic) of labels every call, and both fit the 256 MB Infinity Cache, so ``label_tb_per_s`` is a rate of labels
consumed, largely served from that cache, and not a measurement of HBM traffic; ``of_hbm_spec`` only sets it beside
the 8 TB/s DESIGN.md uses.  In an evaluation loop the labels were just written by the head and are as likely to be
cached.  No profiler trace is taken.  Needs a HIP device; prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import (COCOPanopticEvaluator, PanopticGroundTruth, SemSegEvaluator,  # noqa: E402
                      label_pair_counts_ragged)
from bm2f_amd import _native, label_counts  # noqa: E402

HBM_BYTES_PER_S = 8e12
OFFSET = 256 ** 3


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def best(fn, reps):
    return min(timed(fn, reps) for _ in range(2))


def launch_window_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def blobs(h, w, n, g, dev):
    """An (h, w) int64 map of n elliptical blobs painted in turn over a background of 0: values 0 .. n."""
    y, x = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    out = torch.zeros(h, w, dtype=torch.int64, device=dev)
    c = torch.rand(n, 4, generator=g).tolist()
    for k, (cy, cx, ry, rx) in enumerate(c):
        inside = ((y - cy * h) / (ry * 0.25 * h + 8)) ** 2 + ((x - cx * w) / (rx * 0.25 * w + 8)) ** 2 <= 1
        out[inside] = k + 1
    return out


def kernel_window(a_planes, b_planes, rows, cols, ignore, ids, share, path, reps):
    """The C entry point alone on one flat buffer per side, allocated once -> (ms per call, label bytes)."""
    dev = a_planes[0].device
    G = len(a_planes)
    fa, fb = torch.cat([p.reshape(-1) for p in a_planes]), torch.cat([p.reshape(-1) for p in b_planes])
    pixels = np.array([p.numel() for p in a_planes], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(pixels)))[:-1]
    rows, cols = np.broadcast_to(rows, G).astype(np.int64), np.broadcast_to(cols, G).astype(np.int64)
    bins = rows * cols
    out_off = np.zeros(G, np.int64) if share else np.concatenate(([0], np.cumsum(bins)))[:-1]
    out_len = int(bins[0] if share else bins.sum())
    id_n = np.full(G, -1, np.int64) if ids is None else np.array([len(x) for x in ids], dtype=np.int64)
    id_off = np.zeros(G, np.int64) if ids is None else np.concatenate(([0], np.cumsum(id_n)))[:-1]
    images = np.stack((off, off, pixels, rows, cols, out_off, id_off, id_n), axis=1).astype(np.int64)
    blocks = label_counts._blocks(off, pixels)
    flat_ids = (np.concatenate([np.asarray(x) for x in ids]) if ids else np.zeros(0)).astype(np.int32)
    d = _native.upload_tables({"images": images, "ids": flat_ids, "blocks": blocks}, dev)
    out = torch.zeros(out_len + G, dtype=torch.int64, device=dev)
    args = (fa.data_ptr(), fa.element_size(), fa.numel(), fb.data_ptr(), fb.element_size(), fb.numel(),
            d["images"].data_ptr(), G, _native.ptr_or_null(d["ids"]), flat_ids.size, d["blocks"].data_ptr(),
            blocks.shape[0], int(ignore is not None), ignore or 0, int(bins.max()), {"auto": 0, "lds": 1, "global": 2}[path],
            out.data_ptr(), out_len, out.data_ptr() + 8 * out_len, _native.stream(dev))
    ms = launch_window_ms(lambda: _native.call("m2f_label_pair_counts_ragged", *args), reps)
    return ms, fa.numel() * fa.element_size() + fb.numel() * fb.element_size(), int(blocks.shape[0])


def measure(name, a_planes, b_planes, host_route, kw, a, process_device, process_host):
    """-> the result dict of one shape; the device tables of every path are checked against the host route first."""
    lds_bins = label_counts.geometry()[2]
    max_bins = int(np.max(np.asarray(kw["rows"]) * np.asarray(kw["cols"])))
    paths = ["global"] + (["lds"] if max_bins <= lds_bins else [])
    want = host_route()
    res = {"images": len(a_planes), "pixels": int(sum(p.numel() for p in a_planes)), "max_table_bins": max_bins,
           "auto_picks": "lds" if max_bins <= lds_bins else "global", "host_ms": round(best(host_route, a.reps), 3)}
    for path in paths:
        tables, bad = label_pair_counts_ragged(a_planes, b_planes, path=path, **kw)
        assert not bad.any()
        got = [tables] if kw.get("share_output") else tables
        assert len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want)), f"{name}: {path} differs"
        ms = best(lambda: label_pair_counts_ragged(a_planes, b_planes, path=path, **kw), a.device_reps)
        k_ms, nbytes, wgs = kernel_window(a_planes, b_planes, kw["rows"], kw["cols"], kw.get("ignore"), kw.get("ids"),
                                          kw.get("share_output", False), path, a.kernel_reps)
        res[path] = {"device_ms": round(ms, 3), "host_over_device": round(res["host_ms"] / ms, 2),
                     "kernel": {"launch_window_ms": round(k_ms, 4), "window_reps": a.kernel_reps, "workgroups": wgs,
                                "label_bytes": int(nbytes), "fits_infinity_cache": bool(nbytes < 256 * 2 ** 20),
                                "label_tb_per_s": round(nbytes / k_ms / 1e9, 3),
                                "of_hbm_spec": round(nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4)}}
    if process_device is not None:
        res["process_ms"] = round(best(process_device, a.device_reps), 3)
        res["process_host_ms"] = round(best(process_host, a.reps), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-reps", type=int, default=50, help="calls per window of a device route")
    ap.add_argument("--kernel-reps", type=int, default=100, help="calls inside one device-event window")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_eval_bench: needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    vec, chunk_vecs, lds_bins, max_ids = label_counts.geometry()
    res = {"bench": "seg_eval", "device": torch.cuda.get_device_name(0), "reps": a.reps, "device_reps": a.device_reps,
           "geometry": {"vec": vec, "chunk_vecs": chunk_vecs, "lds_bins": lds_bins, "max_ids": max_ids}}

    # ---- semantic: blob maps and per-pixel random maps ----
    K, H, W, ignore = 150, 512, 683, 255
    for name in ("semantic", "random"):
        if name == "semantic":
            gts = [(blobs(H, W, 12, g, dev) * 11 % K).to(torch.uint8) for _ in range(a.images)]
            preds = [torch.roll(x, (5, 7), (0, 1)).to(torch.int16) for x in gts]
            for x in gts:
                x[:8] = ignore
        else:
            gts = [torch.randint(0, K, (H, W), generator=g).to(torch.uint8).to(dev) for _ in range(a.images)]
            preds = [torch.randint(0, K, (H, W), generator=g).to(torch.int16).to(dev) for _ in range(a.images)]

        def host_sem(gts=gts, preds=preds):
            conf = np.zeros((K + 1, K + 1), dtype=np.int64)
            for x, y in zip(gts, preds):
                gt = x.cpu().numpy().astype(np.int64)
                pred = y.cpu().numpy().astype(np.int64)
                gt[gt == ignore] = K
                conf += np.bincount((K + 1) * pred.reshape(-1) + gt.reshape(-1), minlength=conf.size).reshape(conf.shape)
            return [conf.T.copy()]                                      # [gt, pred], as the kernel counts

        def proc(on_host, gts=gts, preds=preds):
            ev = SemSegEvaluator(K, ignore)
            if on_host:
                ev.process([{"sem_seg": x.cpu()} for x in gts], [{"sem_seg_labels": y.cpu()} for y in preds])
            else:
                ev.process([{"sem_seg": x} for x in gts], [{"sem_seg_labels": y} for y in preds])
            return ev

        kw = dict(rows=K + 1, cols=K + 1, ignore=ignore, share_output=True)
        res[name] = {"shape": [a.images, H, W], "num_classes": K,
                     **measure(name, gts, preds, host_sem, kw, a, lambda: proc(False), lambda: proc(True))}

    # ---- panoptic ----
    H, W, cats, segs = 800, 1216, 133, 40
    categories = [{"id": c + 1, "isthing": int(c < 80)} for c in range(cats)]
    gt_maps, pred_maps, annotations, outputs, id_lists, rows, cols = [], [], [], [], [], [], []
    for i in range(a.images):
        gt = blobs(H, W, segs, g, dev)
        present = torch.unique(gt).tolist()
        gt_ids = {v: 1000 * v + 7 for v in present if v}               # ids that differ from any category
        lut = torch.zeros(segs + 1, dtype=torch.int64, device=dev)
        for v, s in gt_ids.items():
            lut[v] = s
        gt_maps.append(lut[gt].to(torch.int32))
        pred = torch.roll(gt, (9, 13), (0, 1))
        pred_maps.append(pred.to(torch.int32))
        annotations.append({"image_id": i, "file_name": f"{i}.png",
                            "segments_info": [{"id": s, "category_id": (3 * v) % cats + 1, "iscrowd": 0}
                                              for v, s in gt_ids.items()]})
        shown = [v for v in torch.unique(pred).tolist() if v]
        outputs.append({"panoptic_seg": (pred_maps[-1], [{"id": v, "category_id": (3 * v) % cats + 1} for v in shown])})
        id_lists.append([0] + sorted(gt_ids.values()))
        rows.append(len(id_lists[-1]) + 1)
        cols.append(max(shown) + 1)
    js = {"categories": categories, "annotations": annotations}
    inputs = [{"image_id": i} for i in range(a.images)]
    gt_dev = PanopticGroundTruth(js, {i: m for i, m in enumerate(gt_maps)})

    def host_pan():
        out = []
        for i in range(a.images):
            gt, pred = gt_maps[i].cpu().numpy(), pred_maps[i].cpu().numpy()
            labels, counts = np.unique(gt.astype(np.uint64) * OFFSET + pred.astype(np.uint64), return_counts=True)
            table = np.zeros((rows[i], cols[i]), dtype=np.int64)
            r = np.searchsorted(np.asarray(id_lists[i], dtype=np.uint64), labels // OFFSET)
            table[r, (labels % OFFSET).astype(np.int64)] = counts
            out.append(table)
        return out

    def proc_pan(on_host):
        if on_host:
            gt = PanopticGroundTruth(js, {i: m.cpu() for i, m in enumerate(gt_maps)})
            outs = [{"panoptic_seg": (o["panoptic_seg"][0].cpu(), o["panoptic_seg"][1])} for o in outputs]
        else:
            gt, outs = gt_dev, outputs
        ev = COCOPanopticEvaluator(gt, {}, {})
        ev.process(inputs, outs)
        return ev

    kw = dict(rows=rows, cols=cols, ids=id_lists)
    res["panoptic"] = {"shape": [a.images, H, W], "categories": cats, "segments": segs,
                       **measure("panoptic", gt_maps, pred_maps, host_pan, kw, a, lambda: proc_pan(False),
                                 lambda: proc_pan(True))}
    assert proc_pan(False).evaluate()["panoptic_seg"]["stats"] == proc_pan(True).evaluate()["panoptic_seg"]["stats"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
