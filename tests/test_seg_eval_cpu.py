"""The numpy path of the label-pair counts, SemSegEvaluator and COCOPanopticEvaluator, each against an independent
oracle: ``np.bincount`` for the counts, the recorded statistics of the reference's ``pq_compute_single_image``
(tests/golden/gen_seg_eval_golden.py) for semantic PQ, the metric formulas evaluated here for mIoU and the dense
per-pixel restatement tests/pq_ref.py for panoptic PQ.  Counts and tp / fp / fn are integers and compared exactly; the
fp64 ``iou`` sums are compared with ``==`` too: the oracles divide the same two integers and add in the same order
(ascending (ground-truth id, predicted id) within an image, then image by image)."""
import math

import numpy as np
import pytest
import torch

import pq_ref
from bm2f_amd import (COCOPanopticEvaluator, PanopticGroundTruth, SemSegEvaluator, evaluate_panoptic, evaluate_sem_seg,
                      id2rgb, label_pair_counts, label_pair_counts_ragged, pq_from_counts, rgb2id)
from seg_eval_cases import IGNORE_LABEL, NUM_CLASSES, load_fixture, stats_rows


# -------------------------------------------------------------------------------------------------------------------
# label_pair_counts*
# -------------------------------------------------------------------------------------------------------------------
def _bincount_direct(a, b, rows, cols, ignore):
    a, b = a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)
    row = np.full(a.shape, -1, dtype=np.int64)
    ok = (a >= 0) & (a < rows - 1)
    row[ok] = a[ok]
    if ignore is not None:
        row[a == ignore] = rows - 1
    good = (row >= 0) & (b >= 0) & (b < cols)
    table = np.bincount(row[good] * cols + b[good], minlength=rows * cols).reshape(rows, cols)
    return table, int((~good).sum())


def _bincount_ids(a, b, ids, cols):
    a, b = a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)
    rows = len(ids) + 1
    row = np.full(a.shape, rows - 1, dtype=np.int64)
    for j, v in enumerate(ids):
        row[a == v] = j
    good = (b >= 0) & (b < cols)
    table = np.bincount(row[good] * cols + b[good], minlength=rows * cols).reshape(rows, cols)
    return table, int((~good).sum())


@pytest.mark.parametrize("a_dtype", [np.uint8, np.int16, np.int32])
@pytest.mark.parametrize("b_dtype", [np.uint8, np.int16, np.int32, np.int64])
def test_counts_direct_against_bincount(a_dtype, b_dtype):
    rng = np.random.RandomState(0)
    a = rng.randint(0, 7, size=(13, 17)).astype(a_dtype)
    a[2, 3:9] = 99                          # the ignore label
    a[5, 5] = 50                            # neither a class nor the ignore label: bad
    b = rng.randint(0, 6, size=(13, 17)).astype(b_dtype)
    b[7, 7] = 6                             # beyond the columns: bad
    want, want_bad = _bincount_direct(a, b, 8, 6, 99)
    got, bad = label_pair_counts(a, b, rows=8, cols=6, ignore=99)
    assert got.dtype == np.int64 and np.array_equal(got, want) and bad == want_bad == 2
    got_t, bad_t = label_pair_counts(torch.from_numpy(a), torch.from_numpy(b), rows=8, cols=6, ignore=99)
    assert np.array_equal(got_t, want) and bad_t == 2


def test_counts_id_list_against_bincount():
    rng = np.random.RandomState(1)
    ids = [0, 1, 7, 300, 2 ** 24 - 1]
    a = np.array(ids + [5, 9999])[rng.randint(0, 7, size=(9, 31))].astype(np.int32)      # 5 and 9999 are not listed
    b = rng.randint(0, 4, size=(9, 31)).astype(np.int64)
    b[0, 0] = -1
    want, want_bad = _bincount_ids(a, b, ids, 4)
    got, bad = label_pair_counts(a, b, rows=len(ids) + 1, cols=4, ids=ids)
    assert np.array_equal(got, want) and bad == want_bad == 1
    assert got[-1].sum() > 0                                                             # the "other" row is used
    with pytest.raises(ValueError, match="sorted"):
        label_pair_counts(a, b, rows=6, cols=4, ids=[3, 1])
    with pytest.raises(ValueError, match="ids"):
        label_pair_counts(a, b, rows=3, cols=4, ids=[1, 2, 3])


def test_counts_ragged_shared_and_separate():
    rng = np.random.RandomState(2)
    sizes = [(1, 1), (3, 21), (0, 5), (8, 8), (5, 13)]
    a = [rng.randint(0, 5, size=s).astype(np.uint8) for s in sizes]
    b = [rng.randint(0, 6, size=s).astype(np.int16) for s in sizes]
    want = [_bincount_direct(x, y, 6, 6, None)[0] for x, y in zip(a, b)]
    tables, bad = label_pair_counts_ragged(a, b, rows=6, cols=6)
    assert len(tables) == 5 and all(np.array_equal(t, w) for t, w in zip(tables, want)) and not bad.any()
    assert tables[2].sum() == 0                                                          # the zero-pixel image
    shared, bad = label_pair_counts_ragged(a, b, rows=6, cols=6, share_output=True)
    assert np.array_equal(shared, sum(want)) and bad.shape == (5,)
    tables, bad = label_pair_counts_ragged([], [], rows=6, cols=6)
    assert tables == [] and bad.shape == (0,)
    shared, _ = label_pair_counts_ragged([], [], rows=6, cols=6, share_output=True)
    assert shared.shape == (6, 6) and not shared.any()
    with pytest.raises(ValueError, match="pixels"):
        label_pair_counts_ragged([a[0]], [b[1]], rows=6, cols=6)
    with pytest.raises(ValueError, match="uint8, int16 or int32"):
        label_pair_counts_ragged([a[0].astype(np.int64)], [b[0]], rows=6, cols=6)
    with pytest.raises(ValueError, match="path"):
        label_pair_counts_ragged(a, b, rows=6, cols=6, path="fast")


# -------------------------------------------------------------------------------------------------------------------
# semantic: the recorded reference statistics and the metric formulas
# -------------------------------------------------------------------------------------------------------------------
FIXTURE = load_fixture()


def test_pq_ref_reproduces_the_reference_on_the_semantic_fixtures():
    gts, preds, expected = FIXTURE
    categories = {c: {"isthing": 0} for c in range(NUM_CLASSES)}
    per_image = []
    for gt, pred, want in zip(gts, preds, expected["images"]):
        gt_segments = [{"id": int(c), "category_id": int(c), "iscrowd": 0} for c in np.unique(gt) if c != IGNORE_LABEL]
        pred_segments = [{"id": int(c), "category_id": int(c)} for c in np.unique(pred)]
        st = pq_ref.pq_single(gt, gt_segments, pred, pred_segments, categories, void=IGNORE_LABEL, pred_void=None)
        assert stats_rows(st) == stats_rows(want)
        per_image.append(st)
    assert stats_rows(pq_ref.pq_total(per_image)) == stats_rows(expected["total"])


@pytest.mark.parametrize("batch", [1, 4, 16])
def test_sem_seg_pq_equals_the_reference(batch):
    gts, preds, expected = FIXTURE
    ev = SemSegEvaluator(NUM_CLASSES, IGNORE_LABEL, with_pq=True)
    for k in range(0, len(gts), batch):
        ev.process([{"sem_seg": g} for g in gts[k:k + batch]], [{"sem_seg_labels": p} for p in preds[k:k + batch]])
    res = ev.evaluate()["sem_seg"]
    assert stats_rows(res["pq_stats"]) == stats_rows(expected["total"])                  # integers and iou, ==
    for i, want in enumerate(expected["images"]):
        table, _ = label_pair_counts(gts[i], preds[i], rows=NUM_CLASSES + 1, cols=NUM_CLASSES + 1, ignore=IGNORE_LABEL)
        assert stats_rows(ev.image_pq(table).as_dict()) == stats_rows(want)
    pq, sq, rq, n = pq_ref.pq_average({c: r for c, r in enumerate(stats_rows(expected["total"]))},
                                      {c: {"isthing": 0} for c in range(NUM_CLASSES)})
    assert (res["PQ"], res["SQ"], res["RQ"]) == (100 * pq, 100 * sq, 100 * rq) and n == NUM_CLASSES


@pytest.mark.parametrize("count", [1, None], ids=["first", "all"])
def test_sem_seg_metrics_against_the_formulas(count):
    gts, preds = FIXTURE[0][:count], FIXTURE[1][:count]
    K = NUM_CLASSES
    conf = np.zeros((K + 1, K + 1), dtype=np.int64)
    for gt, pred in zip(gts, preds):
        g = gt.astype(np.int64).copy()
        g[g == IGNORE_LABEL] = K
        conf += np.bincount((K + 1) * pred.astype(np.int64).reshape(-1) + g.reshape(-1),
                            minlength=conf.size).reshape(conf.shape)
    names = [f"c{k}" for k in range(K)]
    plain = SemSegEvaluator(K, IGNORE_LABEL, class_names=names)
    plain.process([{"sem_seg": torch.from_numpy(g)} for g in gts],
                  [{"sem_seg_labels": torch.from_numpy(p.astype(np.int16))} for p in preds])
    assert np.array_equal(plain.conf_matrix, conf)                                       # [pred, gt]
    with_pq = SemSegEvaluator(K, IGNORE_LABEL, class_names=names, with_pq=True)
    with_pq.process([{"sem_seg": g} for g in gts], [{"sem_seg_labels": p} for p in preds])
    assert np.array_equal(with_pq.conf_matrix, conf)
    res = plain.evaluate()["sem_seg"]

    tp = conf.diagonal()[:-1].astype(np.float64)
    pos_gt = conf[:-1, :-1].sum(0).astype(np.float64)
    pos_pred = conf[:-1, :-1].sum(1).astype(np.float64)
    acc_valid, iou_valid = pos_gt > 0, pos_gt + pos_pred > 0
    union = pos_gt + pos_pred - tp
    iou = tp[acc_valid] / union[acc_valid]
    acc = tp[acc_valid] / pos_gt[acc_valid]
    assert res["mIoU"] == 100 * (np.sum(iou) / np.sum(iou_valid))
    assert res["mACC"] == 100 * (np.sum(acc) / np.sum(acc_valid))
    assert res["fwIoU"] == 100 * np.sum(iou * (pos_gt / np.sum(pos_gt))[acc_valid])
    assert res["pACC"] == 100 * (np.sum(tp) / np.sum(pos_gt))
    valid = np.flatnonzero(acc_valid)
    for j, k in enumerate(valid):
        assert res[f"IoU-c{k}"] == 100 * iou[j] and res[f"ACC-c{k}"] == 100 * acc[j]
    for k in np.flatnonzero(~acc_valid):
        assert math.isnan(res[f"IoU-c{k}"]) and math.isnan(res[f"ACC-c{k}"])
    if count == 1:      # the hand-made image predicts classes its ground truth lacks: the two denominators differ
        assert np.sum(iou_valid) > np.sum(acc_valid) and (~acc_valid).any()
    assert evaluate_sem_seg(gts, preds, K, IGNORE_LABEL, class_names=names, batch_size=4) == pytest.approx(res, nan_ok=True, rel=0, abs=0)


def test_sem_seg_scores_are_argmaxed_and_bad_labels_refused():
    gts, preds, _ = FIXTURE
    K = NUM_CLASSES
    scores = torch.nn.functional.one_hot(torch.from_numpy(preds[0].astype(np.int64)), K).permute(2, 0, 1).float()
    a = SemSegEvaluator(K, IGNORE_LABEL)
    a.process([{"sem_seg": gts[0]}], [{"sem_seg": scores}])
    b = SemSegEvaluator(K, IGNORE_LABEL)
    b.process([{"sem_seg": gts[0]}], [{"sem_seg_labels": preds[0]}])
    assert np.array_equal(a.conf_matrix, b.conf_matrix)
    bad_gt = gts[1].copy()
    bad_gt[0, 0] = K + 3                                                                  # no class, not the ignore label
    ev = SemSegEvaluator(K, IGNORE_LABEL)
    with pytest.raises(ValueError, match="file_name 'second.png'"):
        ev.process([{"sem_seg": gts[0], "file_name": "first.png"}, {"sem_seg": bad_gt, "file_name": "second.png"}],
                   [{"sem_seg_labels": preds[0]}, {"sem_seg_labels": preds[1]}])
    bad_pred = preds[1].astype(np.int16)
    bad_pred[0, 0] = -1
    with pytest.raises(ValueError, match="predicted label"):
        SemSegEvaluator(K, IGNORE_LABEL).process([{"sem_seg": gts[1]}], [{"sem_seg_labels": bad_pred}])
    top_pred = preds[1].copy()
    top_pred[0, 0] = K                                                                    # the column kept empty
    for with_pq in (False, True):
        with pytest.raises(ValueError, match=f"image_id 'b'.*predicted label {K}"):
            SemSegEvaluator(K, IGNORE_LABEL, with_pq=with_pq).process(
                [{"sem_seg": gts[0], "image_id": "a"}, {"sem_seg": gts[1], "image_id": "b"}],
                [{"sem_seg_labels": preds[0]}, {"sem_seg_labels": top_pred}])


def test_sem_seg_file_name_route(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    gts, preds, _ = FIXTURE
    path = str(tmp_path / "gt.png")
    Image.fromarray(gts[0]).save(path)
    a = SemSegEvaluator(NUM_CLASSES, IGNORE_LABEL)
    a.process([{"sem_seg_file_name": path}], [{"sem_seg_labels": preds[0]}])
    b = SemSegEvaluator(NUM_CLASSES, IGNORE_LABEL)
    b.process([{"sem_seg": gts[0]}], [{"sem_seg_labels": preds[0]}])
    assert np.array_equal(a.conf_matrix, b.conf_matrix)


# -------------------------------------------------------------------------------------------------------------------
# panoptic: hand-made images against the dense restatement
# -------------------------------------------------------------------------------------------------------------------
CATEGORIES = [{"id": 1, "name": "person", "isthing": 1}, {"id": 2, "name": "car", "isthing": 1},
              {"id": 3, "name": "sky", "isthing": 0}, {"id": 4, "name": "road", "isthing": 0}]
THINGS, STUFF = {1: 0, 2: 1}, {3: 2, 4: 3}            # dataset id -> the head's contiguous id
CAT = {c["id"]: c for c in CATEGORIES}
BIG = 2 ** 24 - 1


def _seg(i, cat, crowd=0):
    return {"id": i, "category_id": cat, "iscrowd": crowd}


def _head(i, cat):
    """A predicted segment as the head lists it: a contiguous category id and isthing."""
    thing = bool(CAT[cat]["isthing"])
    return {"id": i, "isthing": thing, "category_id": (THINGS if thing else STUFF)[cat]}


def panoptic_images():
    """{image_id: (gt_map, gt_segments, pred_map, head segments, dataset-id segments)}"""
    out = {}
    # a: an unmatched prediction lying on a crowd of its category is spared; the stuff below is matched (IoU 0.8)
    gt = np.zeros((8, 8), np.int32)
    gt[:4], gt[4:] = 10, 20
    pred = np.zeros((8, 8), np.int32)
    pred[:3], pred[3:] = 1, 2
    out["a"] = (gt, [_seg(10, 1, crowd=1), _seg(20, 3)], pred, [(1, 1), (2, 3)])
    # b: two crowds of one category, listed 5 then 3: the last one (3) is the one remembered, so the prediction on
    # crowd 5 is a counted fp and the one on crowd 3 is spared; ids differ from categories and from their order
    gt = np.zeros((6, 12), np.int32)
    gt[:, :4], gt[:, 4:8], gt[:, 8:] = 5, 3, BIG
    pred = np.zeros((6, 12), np.int32)
    pred[:, :4], pred[:, 4:8], pred[:, 8:] = 1, 2, 7
    out["b"] = (gt, [_seg(5, 1, crowd=1), _seg(3, 1, crowd=1), _seg(BIG, 4)], pred, [(1, 1), (2, 1), (7, 4)])
    # c: a prediction exactly half on VOID is not spared; IoU exactly 0.5 is not matched (fn and fp); VOID in the
    # prediction; ground-truth pixels of an unlisted id (the "other" row) count for the prediction's area only
    gt = np.full((4, 8), 30, np.int32)
    gt[0] = 0                                           # VOID
    gt[3, :2] = 40                                      # two pixels of sky
    gt[3, 6:] = 99                                      # not listed
    pred = np.full((4, 8), 3, np.int32)
    pred[:2] = 1                                        # 16 pixels, 8 of them on VOID
    pred[3, 0] = 2                                      # one of the two sky pixels: inter 1, union 2
    pred[3, 7] = 0                                      # VOID in the prediction
    out["c"] = (gt, [_seg(30, 4), _seg(40, 3)], pred, [(1, 2), (2, 3), (3, 4)])
    return {k: (g, gs, p, [_head(i, c) for i, c in ps], [{"id": i, "category_id": c} for i, c in ps])
            for k, (g, gs, p, ps) in out.items()}


IMAGES = panoptic_images()


def _ground_truth(images=IMAGES, device_maps=None):
    js = {"categories": CATEGORIES,
          "annotations": [{"image_id": k, "file_name": f"{k}.png", "segments_info": v[1]} for k, v in images.items()]}
    return PanopticGroundTruth(js, id_maps=device_maps or {k: v[0] for k, v in images.items()})


def _reference(images=IMAGES):
    per_image = {k: pq_ref.pq_single(v[0], v[1], v[2], v[4], CAT, image_id=k) for k, v in images.items()}
    return per_image, pq_ref.pq_total(list(per_image.values()))


def _rows(stats):
    return [[stats[c][k] if not isinstance(stats[c], dict) else stats[c][n]
             for k, n in enumerate(("tp", "fp", "fn", "iou"))] for c in sorted(CAT)]


def test_panoptic_cases_hold_what_they_claim():
    per_image, total = _reference()
    assert per_image["a"][1] == [0, 0, 0, 0.0] and per_image["a"][3] == [1, 0, 0, 0.8]   # spared by the crowd
    assert per_image["b"][1] == [0, 1, 0, 0.0] and per_image["b"][4] == [1, 0, 0, 1.0]   # the last crowd wins
    assert per_image["c"][2] == [0, 1, 0, 0.0]                                           # exactly half VOID: counted
    assert per_image["c"][3] == [0, 1, 1, 0.0]                                           # IoU exactly 0.5: not matched
    assert per_image["c"][4][0] == 1 and 0.5 < per_image["c"][4][3] < 1.0
    assert total[3][0] == 1 and total[3][1] == 1                                         # sky predicted in two images


@pytest.mark.parametrize("tensors", [False, True])
def test_panoptic_evaluator_against_pq_ref(tensors):
    per_image, total = _reference()
    gt = _ground_truth()
    ev = COCOPanopticEvaluator(gt, THINGS, STUFF)
    keys = list(IMAGES)
    wrap = torch.from_numpy if tensors else (lambda x: x)
    ev.process([{"image_id": k} for k in keys[:2]], [{"panoptic_seg": (wrap(IMAGES[k][2]), IMAGES[k][3])} for k in keys[:2]])
    ev.process([{"image_id": keys[2]}], [{"panoptic_seg": (wrap(IMAGES[keys[2]][2]), IMAGES[keys[2]][3])}])
    res = ev.evaluate()["panoptic_seg"]
    assert _rows(res["stats"]) == _rows(total)
    for suffix, isthing in (("", None), ("_th", True), ("_st", False)):
        pq, sq, rq, n = pq_ref.pq_average(total, CAT, isthing)
        assert (res["PQ" + suffix], res["SQ" + suffix], res["RQ" + suffix]) == (100 * pq, 100 * sq, 100 * rq)
        assert res["n" + suffix] == n
    assert set(res["per_class"]) == set(CAT)
    # the functional form, with dataset ids, and one table at a time
    again = evaluate_panoptic(gt, [(k, v[2], v[4]) for k, v in IMAGES.items()], batch_size=2)
    assert again["stats"] == res["stats"] and again["PQ"] == res["PQ"]
    for k, (g, gs, p, _, ps) in IMAGES.items():
        order = sorted(range(len(gs)), key=lambda i: gs[i]["id"])
        ids = [0] + [gs[i]["id"] for i in order]
        table, bad = label_pair_counts(g, p, rows=len(ids) + 1, cols=int(p.max()) + 1, ids=ids)
        rows = np.zeros(len(gs), np.int64)
        rows[order] = np.arange(1, len(gs) + 1)
        assert bad == 0 and _rows(pq_from_counts(table, gs, ps, CAT, gt_rows=rows).as_dict()) == _rows(per_image[k])


def test_panoptic_empty_things_group_is_nan():
    gt = np.full((4, 4), 20, np.int32)
    pred = np.full((4, 4), 2, np.int32)
    images = {"s": (gt, [_seg(20, 3)], pred, [_head(2, 3)], [{"id": 2, "category_id": 3}])}
    ev = COCOPanopticEvaluator(_ground_truth(images), THINGS, STUFF)
    ev.process([{"image_id": "s"}], [{"panoptic_seg": (pred, images["s"][3])}])
    res = ev.evaluate()["panoptic_seg"]
    assert res["n_th"] == 0 and all(math.isnan(res[k]) for k in ("PQ_th", "SQ_th", "RQ_th"))
    assert res["PQ"] == res["PQ_st"] == 100.0 and res["n"] == 1


def test_panoptic_key_errors():
    g, gs, p, hs, _ = IMAGES["a"]
    gt = _ground_truth()

    def run(pred, segs):
        ev = COCOPanopticEvaluator(gt, THINGS, STUFF)
        ev.process([{"image_id": "a"}], [{"panoptic_seg": (pred, segs)}])

    extra = p.copy()
    extra[0, 0] = 9                                     # pixels of an id that segments_info does not list
    with pytest.raises(KeyError, match="segment with ID 9 is presented in PNG and not presented in JSON"):
        run(extra, hs)
    with pytest.raises(KeyError, match=r"segment IDs \[5\] are presented in JSON and not presented in PNG"):
        run(p, hs + [_head(5, 3)])                      # listed, without a pixel
    with pytest.raises(KeyError, match="segment with ID 2 has unknown category_id 77"):
        run(p, [hs[0], {"id": 2, "category_id": 77}])   # no isthing: already a dataset id
    unlisted_low = p.copy()
    unlisted_low[:3] = 1
    with pytest.raises(KeyError, match="segment with ID 1 is presented in PNG"):
        run(unlisted_low, [hs[1]])
    rgb_style = np.where(p == 1, 2 ** 20, p).astype(np.int32)      # one column per id would be a table of 2^20 columns
    with pytest.raises(ValueError, match="predicted ids must stay below"):
        run(rgb_style, [{**hs[0], "id": 2 ** 20}, hs[1]])
    with pytest.raises(KeyError, match="mapping does not hold"):
        run(p, [hs[0], {"id": 2, "isthing": False, "category_id": 99}])


def test_rgb2id_roundtrip_and_png_ground_truth(tmp_path):
    ids = np.array([[0, 1, 255], [256, 65536, BIG]], dtype=np.int32)
    rgb = id2rgb(ids)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb2id(rgb), ids)
    assert id2rgb(BIG) == [255, 255, 255] and rgb2id([1, 2, 3]) == 1 + 2 * 256 + 3 * 65536
    Image = pytest.importorskip("PIL.Image")
    g, gs, p, hs, _ = IMAGES["b"]
    Image.fromarray(id2rgb(g)).save(str(tmp_path / "b.png"))
    js = {"categories": CATEGORIES, "annotations": [{"image_id": "b", "file_name": "b.png", "segments_info": gs}]}
    ev = COCOPanopticEvaluator(PanopticGroundTruth(js, png_root=str(tmp_path)), THINGS, STUFF)
    ev.process([{"image_id": "b"}], [{"panoptic_seg": (p, hs)}])
    assert _rows(ev.evaluate()["panoptic_seg"]["stats"]) == _rows(_reference({"b": IMAGES["b"]})[1])
