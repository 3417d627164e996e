"""The label-map RLE cases shared by tests/test_label_rle_cpu.py and tests/test_label_rle_gpu.py, the literal
per-value references they are compared with, and the checks of the public pieces, which take the device as an
argument.  Everything here is integer-exact: every comparison is equality."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import torch

from bm2f_amd import (SemSegEvaluator, evaluate_sem_seg, instance_map_annotations, label_maps_to_rle,
                      load_sem_seg_predictions, panoptic_to_coco_detection, rle_encode, rle_to_label_maps,
                      sem_seg_to_coco_json)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "evaluate_pq_for_semantic_segmentation.py")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, labels, dtype, seed):
    """A plane of `labels` distinct values drawn per pixel."""
    return torch.randint(0, labels, shape, generator=_gen(seed)).to(dtype)


def _blobs(shape, labels, dtype, seed):
    """Connected regions: labels drawn at an eighth of the resolution and repeated."""
    h, w = shape
    low = torch.randint(0, labels, ((h + 7) // 8, (w + 7) // 8), generator=_gen(seed))
    return low.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w].to(dtype).contiguous()


def _plane(h, w, dtype, pixels, base=0):
    m = torch.full((h, w), base, dtype=dtype)
    for (y, x), v in pixels.items():
        m[y, x] = v
    return m


def _values(shape, values, dtype, seed):
    idx = torch.randint(0, len(values), shape, generator=_gen(seed))
    return torch.tensor(values, dtype=torch.int64)[idx].to(dtype)


def _checker(h, w, labels):
    return ((torch.arange(h)[:, None] + torch.arange(w)[None]) % labels).to(torch.uint8)


def _build():
    """name -> (planes, keyword arguments of label_maps_to_rle); a crop view is kept as a view."""
    c = {}
    c["1x1"] = ([torch.tensor([[5]], dtype=torch.int32)], {})
    c["1x33"] = ([_rand((1, 33), 3, torch.uint8, 1)], {})
    c["33x1"] = ([_rand((33, 1), 3, torch.uint8, 2)], {})
    c["one_label"] = ([torch.full((9, 40), 7, dtype=torch.uint8)], {})            # counts decode to [0, N]
    c["owns_pixel0"] = ([_plane(9, 40, torch.uint8, {(0, 0): 3})], {})
    c["last_run_ends_at_HW"] = ([_plane(9, 40, torch.uint8, {(8, 39): 4})], {})
    # a run of label 2 from the last row of column x into the first row of column x + 1: no transition there
    c["run_crosses_columns"] = ([_plane(9, 40, torch.int16, {(7, 31): 2, (8, 31): 2, (0, 32): 2, (1, 32): 2,
                                                             (8, 5): 2, (0, 6): 2})], {})
    # the reverse: the last row is set and the next column's first row holds another label
    c["run_ends_at_column_end"] = ([_plane(9, 40, torch.int16, {(8, 31): 2, (0, 32): 3, (8, 39): 2, (8, 0): 2,
                                                                (0, 1): 3})], {})
    for h in (7, 9):
        for w in (32, 33, 64, 65, 257):
            for labels, dtype in ((2, torch.uint8), (3, torch.int16), (150, torch.int32)):
                c[f"{h}x{w}_{labels}labels"] = ([_rand((h, w), labels, dtype, 100 * h + w + labels)], {})
    c["33x65_checker2"] = ([_checker(33, 65, 2)], {})
    c["33x65_checker3"] = ([_checker(33, 65, 3)], {})
    c["40x40_every_pixel"] = ([torch.randperm(1600, generator=_gen(3)).view(40, 40).to(torch.int32)], {})
    c["int16_signed"] = ([_values((9, 40), [-1, 0, 32767, -32768], torch.int16, 4)], {})
    c["int32_signed"] = ([_values((9, 40), [-1, 2 ** 24 + 5, 2 ** 31 - 1, -2 ** 31, 0], torch.int32, 5)], {})
    c["uint8_ignore255"] = ([_values((9, 40), [0, 1, 255, 17], torch.uint8, 6)], {"ignore": 255})
    ids_plane = _values((9, 40), [0, 1, 255, 17, 90], torch.uint8, 7)
    c["ids_not_ascending"] = ([ids_plane], {"ids": [[90, 0, 17]]})
    c["ids_absent"] = ([ids_plane], {"ids": [[1, 33, 300, -4, 17]]})
    c["ids_equal_ignore"] = ([ids_plane], {"ids": [[255, 1]], "ignore": 255})
    c["ids_empty"] = ([ids_plane], {"ids": [[]]})
    c["ids_repeated"] = ([ids_plane], {"ids": [[17, 17, 0]]})
    wide = _values((9, 40), [-1, 2 ** 24 + 5, 2 ** 31 - 1, 3], torch.int32, 8)
    c["ids_signed"] = ([wide], {"ids": [[2 ** 31 - 1, -1, 2 ** 24 + 5, 2 ** 24 + 6, 2 ** 40]]})
    batch = [_rand((3, 700), 4, torch.uint8, 9), torch.full((9, 40), 255, dtype=torch.uint8),
             _blobs((130, 300), 150, torch.uint8, 10)]
    c["batch_scalar_ignore"] = (batch, {"ignore": 255})
    per_image = [batch[0], torch.full((9, 40), 3, dtype=torch.uint8), batch[2]]
    c["batch_per_image_ignore"] = (per_image, {"ignore": [0, 3, None]})
    c["batch_ids"] = (batch, {"ignore": 255, "ids": [[3, 0], [255, 4], [149, 7, 200]]})
    c["batch_with_empty_plane"] = ([batch[0], torch.zeros((0, 5), dtype=torch.uint8), batch[1]], {})
    c["crop_view"] = ([_rand((13, 50), 5, torch.int16, 11)[2:11, 3:43]], {})
    c["1056x1000_one_label"] = ([torch.full((1056, 1000), 9, dtype=torch.uint8)], {})   # a count of five characters
    return c


CASES = _build()


def to_device(planes, device):
    """The planes on `device`; a view of a larger buffer stays one (its base is moved, then sliced again)."""
    out = []
    for p in planes:
        if p._base is None:
            out.append(p.to(device))
        else:
            out.append(torch.as_strided(p._base.to(device), p.shape, p.stride(), p.storage_offset()))
    return out


def literal(planes, ignore=None, ids=None):
    """The loops of encode_json_sem_seg and of the ADE script, value by value: rle_encode(plane == v), numpy count
    and box."""
    out = []
    for i, p in enumerate(planes):
        a = p.numpy().astype(np.int64)
        ign = ignore[i] if isinstance(ignore, (list, tuple)) else ignore
        values = ids[i] if ids is not None else [int(v) for v in np.unique(a) if ign is None or v != ign]
        one = []
        for v in values if a.size else []:
            mask = (a == v) if (ign is None or v != ign) else np.zeros_like(a, dtype=bool)
            rle = rle_encode(torch.from_numpy(mask))[0]
            inds = np.nonzero(mask)
            box = [0, 0, 0, 0]
            if inds[0].size:
                ymin, ymax, xmin, xmax = inds[0].min(), inds[0].max(), inds[1].min(), inds[1].max()
                box = [int(xmin), int(ymin), int(xmax - xmin + 1), int(ymax - ymin + 1)]
            one.append({"label": int(v), "segmentation": rle, "area": int(mask.sum()), "bbox": box})
        out.append(one)
    return out


@functools.lru_cache(maxsize=None)
def definition(name):
    """label_maps_to_rle on the CPU, once per case."""
    planes, kw = CASES[name]
    return label_maps_to_rle(planes, **kw)


def painted_back(name, device):
    """(got, want): the planes of a case encoded (every label but the ignored one) and painted again on `device`, and
    the planes themselves with 0 standing in for the ignored pixels."""
    planes, kw = CASES[name]
    ignore = kw.get("ignore")
    dev_planes = to_device(planes, device)
    segs = label_maps_to_rle(dev_planes, ignore=ignore)
    got = rle_to_label_maps([[(e["label"], e["segmentation"]) for e in one] for one in segs],
                            [tuple(p.shape) for p in planes], fill=0, dtype=planes[0].dtype, device=device)
    want = []
    for i, p in enumerate(planes):
        ign = ignore[i] if isinstance(ignore, list) else ignore
        w = p.clone()
        if ign is not None:
            w[p == ign] = 0
        want.append(w)
    return got, want


# -------------------------------------------------------------------------------------------------------------------
# the public pieces, on any device
# -------------------------------------------------------------------------------------------------------------------
def check_painter(device):
    am, bm = torch.zeros(6, 7, dtype=torch.bool), torch.zeros(6, 7, dtype=torch.bool)
    am[1:4, 2] = True
    bm[2:5, 1:4] = True                                                    # overlaps am in two pixels
    a, b = rle_encode(torch.stack((am, bm)))
    for order, top in ((((5, a), (9, b)), 9), (((9, b), (5, a)), 5)):     # the later segment wins
        got, = rle_to_label_maps([list(order)], [(6, 7)], fill=1, dtype=torch.int16, device=device)
        want = torch.full((6, 7), 1, dtype=torch.int16)
        for v, mask in ((5, am), (9, bm)) if top == 9 else ((9, bm), (5, am)):
            want[mask] = v
        assert got.dtype == torch.int16 and torch.equal(got.cpu(), want)
    # the uncompressed list, an image without segments, and the three output dtypes
    listed = {"size": [6, 7], "counts": [8, 3, 31]}
    for dtype, fill, value in ((torch.uint8, 255, 200), (torch.int16, -7, -32768), (torch.int32, 0, 2 ** 31 - 1)):
        got = rle_to_label_maps([[(value, listed)], [], [(value, a)]], [(6, 7), (4, 3), (6, 7)], fill=fill,
                                dtype=dtype, device=device)
        flat = torch.full((42,), fill, dtype=dtype)
        flat[8:11] = value                                                 # column-major pixels 8, 9, 10
        want = flat.view(7, 6).T
        assert [g.dtype for g in got] == [dtype] * 3
        assert torch.equal(got[0].cpu(), want)
        assert torch.equal(got[1].cpu(), torch.full((4, 3), fill, dtype=dtype))
        assert torch.equal(got[2].cpu(), torch.where(am, torch.tensor(value, dtype=dtype), torch.tensor(fill, dtype=dtype)))
    assert rle_to_label_maps([], [], device=device) == []


def check_sem_seg_json(device):
    maps = [_blobs((37, 53), 6, torch.uint8, 20), _rand((9, 40), 4, torch.uint8, 21), _blobs((64, 31), 6, torch.uint8, 22)]
    names = ["val/a_0001.png", "b.with.dots.jpg", "/abs/dir/c.png"]
    ids = ["a_0001", "b", "c"]
    to_dataset = {k: 10 * k + 3 for k in range(6)}
    for mapping in (None, to_dataset):
        entries = sem_seg_to_coco_json(to_device(maps, device), names, contiguous_id_to_dataset_id=mapping)
        want = [(n, (mapping[e["label"]] if mapping else e["label"]), e["segmentation"])
                for n, one in zip(names, literal(maps)) for e in one]
        assert [(e["file_name"], e["category_id"], e["segmentation"]) for e in entries] == want
        back = load_sem_seg_predictions(json.loads(json.dumps(entries)), {i: tuple(m.shape) for i, m in zip(ids, maps)},
                                        dataset_id_to_contiguous_id=None if mapping is None else
                                        {v: k for k, v in mapping.items()}, device=device)
        assert list(back) == ids
        for i, m in zip(ids, maps):
            assert back[i].dtype == torch.int32 and torch.equal(back[i].cpu(), m.to(torch.int32))


def load_tool():
    spec = importlib.util.spec_from_file_location("evaluate_pq_for_semantic_segmentation", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_evaluator(device, tmp_path):
    import seg_eval_cases as sc
    gts, preds, _ = sc.load_fixture()
    inputs = [{"sem_seg": g, "file_name": f"images/img_{i:03d}.png"} for i, g in enumerate(gts)]
    outputs = [{"sem_seg_labels": torch.from_numpy(p)} for p in preds]
    plain = SemSegEvaluator(sc.NUM_CLASSES, sc.IGNORE_LABEL, device=device, with_pq=True)
    keeping = SemSegEvaluator(sc.NUM_CLASSES, sc.IGNORE_LABEL, device=device, with_pq=True, keep_predictions=True,
                              output_dir=str(tmp_path))
    for ev in (plain, keeping):
        for k in range(0, len(inputs), 3):
            ev.process(inputs[k:k + 3], outputs[k:k + 3])
    assert plain.predictions == []
    np.testing.assert_equal(keeping.evaluate(), plain.evaluate())
    with open(os.path.join(str(tmp_path), "sem_seg_predictions.json")) as f:
        written = json.load(f)
    assert written == keeping.predictions
    assert [(e["file_name"], e["category_id"], e["segmentation"]) for e in written] == [
        (inp["file_name"], e["label"], e["segmentation"])
        for inp, one in zip(inputs, literal([torch.from_numpy(p) for p in preds])) for e in one]
    # the written file, read back by the tool's function, counts what the evaluator counted
    again = load_tool().evaluate_predictions(written, {f"img_{i:03d}": g for i, g in enumerate(gts)}, sc.NUM_CLASSES,
                                             sc.IGNORE_LABEL, device=device)
    assert np.array_equal(again.conf_matrix, plain.conf_matrix)
    assert again.pq_stat.as_dict() == plain.pq_stat.as_dict()


def check_tool(device, tmp_path):
    from PIL import Image
    gts = [_blobs((40, 56), 4, torch.uint8, 30), _blobs((33, 47), 4, torch.uint8, 31)]
    gts[0][:5, :9] = 255
    preds = [_blobs((40, 56), 4, torch.uint8, 32), gts[1].clone()]
    preds[1][10:20, 5:30] = 2
    os.makedirs(os.path.join(str(tmp_path), "gt"))
    for name, g in zip(("first", "second"), gts):
        Image.fromarray(g.numpy(), mode="L").save(os.path.join(str(tmp_path), "gt", name + ".png"))
    path = os.path.join(str(tmp_path), "sem_seg_predictions.json")
    with open(path, "w") as f:
        json.dump(sem_seg_to_coco_json(preds, ["x/first.jpg", "x/second.jpg"]), f)
    cmd = [sys.executable, TOOL, "--json-file", path, "--gt-dir", os.path.join(str(tmp_path), "gt"), "--num-classes", "4",
           "--ignore-label", "255"] + (["--device", str(device)] if torch.device(device).type == "cuda" else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.splitlines()
    want = evaluate_sem_seg([g.numpy() for g in gts], [p.numpy() for p in preds], 4, 255, with_pq=True)
    assert [l for l in out if l.startswith("mIoU: ")] == [f"mIoU: {want['mIoU'] / 100}"]
    row = "".join(f"{want[k]:7.1f}" for k in ("PQ", "SQ", "RQ")) + f"{4:7d}"
    assert [l for l in out if l.startswith("All")] == [f"{'All':<10}|{row}"]
    assert [l for l in out if l.startswith("Stuff")] == [f"{'Stuff':<10}|{row}"]


def check_panoptic_to_detection(device):
    id_map = _values((37, 53), [0, 5, 2 ** 24 + 1, 70000, 12], torch.int32, 40)
    id_map = id_map.repeat_interleave(3, 0).repeat_interleave(2, 1).contiguous()
    info = [{"id": 70000, "category_id": 3, "iscrowd": 0}, {"id": 5, "category_id": 1, "iscrowd": 1},
            {"id": 999, "category_id": 2}, {"id": 2 ** 24 + 1, "category_id": 1}]
    cats = [{"id": 1, "isthing": 1}, {"id": 2, "isthing": 0}, {"id": 3, "isthing": 0}]
    for things_only in (False, True):
        got = panoptic_to_coco_detection(17, id_map.to(device), info, first_id=100, things_only=things_only,
                                         categories=cats)
        keep = [s for s in info if not things_only or s["category_id"] == 1]
        ref, = literal([id_map], ids=[[s["id"] for s in keep]])
        want = [{"id": 100 + k, "image_id": 17, "category_id": s["category_id"], "iscrowd": s.get("iscrowd", 0),
                 "bbox": r["bbox"], "area": r["area"], "segmentation": r["segmentation"]}
                for k, (s, r) in enumerate(zip(keep, ref))]
        assert got == want


def ade_planes():
    ids = _blobs((48, 64), 7, torch.uint8, 50)
    cats = (ids * 3 + 1) * (ids > 0)                                       # one category per instance; 0 under VOID
    cats[ids == 0] = _blobs((48, 64), 3, torch.uint8, 51)[ids == 0]        # VOID lies under several categories
    return ids, cats.to(torch.uint8)


def check_instance_map(device):
    ids, cats = ade_planes()
    cat_map = {k: 100 + k for k in range(256)}
    got = instance_map_annotations(ids.to(device), cats.to(device), "ADE_val_1", cat_map=cat_map, first_id=7)
    want, ann_id = [], 7
    a, c = ids.numpy(), cats.numpy()
    for thing in np.unique(a):                                             # the loop of the script
        if thing == 0:
            continue
        mask = a == thing
        cat = np.unique(c[mask])
        assert len(cat) == 1
        inds = np.nonzero(mask)
        ymin, ymax, xmin, xmax = inds[0].min(), inds[0].max(), inds[1].min(), inds[1].max()
        want.append({"id": ann_id, "image_id": "ADE_val_1", "iscrowd": 0, "category_id": cat_map[int(cat[0])],
                     "bbox": [int(xmin), int(ymin), int(xmax - xmin + 1), int(ymax - ymin + 1)],
                     "segmentation": rle_encode(torch.from_numpy(mask))[0], "area": int(mask.sum())})
        ann_id += 1
    assert got == want


def check_errors(device):
    import pytest
    p8, p16 = torch.zeros(4, 5, dtype=torch.uint8, device=device), torch.zeros(4, 5, dtype=torch.int16, device=device)
    with pytest.raises(ValueError, match="different dtypes"):
        label_maps_to_rle([p8, p16])
    with pytest.raises(ValueError, match="uint8, int16 or int32"):
        label_maps_to_rle([p8.float()])
    huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2 ** 16, 2 ** 15)    # a view: nothing is allocated
    with pytest.raises(ValueError, match="32-bit count"):
        label_maps_to_rle([huge])
    rle = rle_encode(torch.ones(4, 5, dtype=torch.bool))[0]
    with pytest.raises(ValueError, match="size"):
        rle_to_label_maps([[(1, rle)]], [(5, 4)], device=device)
    with pytest.raises(ValueError, match="does not fit"):
        rle_to_label_maps([[(256, rle)]], [(4, 5)], dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match="does not fit"):
        rle_to_label_maps([[(-32769, rle)]], [(4, 5)], dtype=torch.int16, device=device)
    with pytest.raises(ValueError, match="not in contiguous_id_to_dataset_id"):
        sem_seg_to_coco_json([p8 + 3], ["a.png"], contiguous_id_to_dataset_id={0: 1, 1: 2})
    ids, cats = ade_planes()
    cats[:24][ids[:24] == 2] += 1                                          # instance 2 now lies under two categories
    assert len(np.unique(cats[ids == 2].numpy())) == 2
    with pytest.raises(ValueError, match="instance 2 lies under"):
        instance_map_annotations(ids.to(device), cats.to(device), 0)
