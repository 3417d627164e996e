"""SemSegEvaluator and COCOPanopticEvaluator fed by MaskFormerInference on the device: the results of the semantic
(``semantic_labels=True``) and panoptic heads stay on the device and are counted there; the same results copied to the
host go through the numpy path.  The host arithmetic on the tables is the same, so every number is compared with
``==``.  The committed semantic fixtures, evaluated from device tensors, must give the reference's recorded counters."""
import math

import numpy as np
import pytest
import torch

from bm2f_amd import COCOPanopticEvaluator, MaskFormerInference, PanopticGroundTruth, SemSegEvaluator
from seg_eval_cases import IGNORE_LABEL, NUM_CLASSES, load_fixture, stats_rows

pytestmark = pytest.mark.gpu

B, Q, K = 2, 8, 5
PADDED = (64, 96)
IMAGE_SIZES = [(60, 90), (50, 96)]
THINGS, STUFF = {11: 0, 12: 1, 13: 2}, {21: 3, 22: 4}                 # dataset id -> contiguous id
CATEGORIES = [{"id": d, "isthing": 1} for d in THINGS] + [{"id": d, "isthing": 0} for d in STUFF]


def _equal(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _equal(a[k], b[k])
    elif isinstance(a, float) and math.isnan(a):
        assert math.isnan(b)
    else:
        assert a == b


@pytest.fixture(scope="module")
def head_results(device):
    g = torch.Generator().manual_seed(0)
    outputs = {"pred_logits": (6 * torch.randn(B, Q, K + 1, generator=g)).to(device),
               "pred_masks": (4 * torch.randn(B, Q, 16, 24, generator=g)).to(device)}
    head = MaskFormerInference(num_classes=K, thing_classes=THINGS.values(), semantic_on=True, panoptic_on=True,
                               object_mask_threshold=0.3, overlap_threshold=0.5)
    results = head(outputs, PADDED, IMAGE_SIZES, semantic_labels=True)
    assert all(r["sem_seg_labels"].device.type == "cuda" and r["panoptic_seg"][0].device.type == "cuda"
               for r in results)
    assert sum(len(r["panoptic_seg"][1]) for r in results) >= 2, "the seeded logits must keep some segments"
    return results


def _blocks(h, w, values, seed, step=10):
    """A label map of step x step blocks drawn from ``values``."""
    rng = np.random.RandomState(seed)
    grid = rng.choice(values, size=((h + step - 1) // step, (w + step - 1) // step))
    return np.kron(grid, np.ones((step, step), dtype=np.int64))[:h, :w]


def test_sem_seg_device_equals_host(head_results, device):
    gts = [_blocks(h, w, [0, 1, 2, 3, 4, IGNORE_LABEL], 20 + i).astype(np.uint8) for i, (h, w) in enumerate(IMAGE_SIZES)]
    for with_pq in (False, True):
        on_device = SemSegEvaluator(K, IGNORE_LABEL, with_pq=with_pq)
        on_device.process([{"sem_seg": torch.from_numpy(x).to(device)} for x in gts], head_results)
        uploaded = SemSegEvaluator(K, IGNORE_LABEL, with_pq=with_pq, device=device)     # host ground truth goes up
        uploaded.process([{"sem_seg": x} for x in gts], head_results)
        on_host = SemSegEvaluator(K, IGNORE_LABEL, with_pq=with_pq)
        on_host.process([{"sem_seg": x} for x in gts], [{"sem_seg_labels": r["sem_seg_labels"].cpu()} for r in head_results])
        assert on_host.conf_matrix.sum() == sum(h * w for h, w in IMAGE_SIZES)
        for ev in (on_device, uploaded):
            assert np.array_equal(ev.conf_matrix, on_host.conf_matrix)
            _equal(ev.evaluate(), on_host.evaluate())


def test_panoptic_device_equals_host(head_results, device):
    annotations, id_maps = [], {}
    for i, (h, w) in enumerate(IMAGE_SIZES):
        id_map = _blocks(h, w, [0, 3, 7, 2 ** 24 - 1, 500, 99], 30 + i, step=16).astype(np.int32)   # 99 is not listed
        segs = [{"id": 3, "category_id": 11, "iscrowd": 0}, {"id": 7, "category_id": 21, "iscrowd": 0},
                {"id": 2 ** 24 - 1, "category_id": 22, "iscrowd": 0}, {"id": 500, "category_id": 12, "iscrowd": 1}]
        annotations.append({"image_id": i, "file_name": f"{i}.png",
                            "segments_info": [s for s in segs if (id_map == s["id"]).any()]})
        id_maps[i] = id_map
    js = {"categories": CATEGORIES, "annotations": annotations}
    inputs = [{"image_id": i} for i in range(B)]
    on_host = COCOPanopticEvaluator(PanopticGroundTruth(js, id_maps), THINGS, STUFF)
    on_host.process(inputs, [{"panoptic_seg": (r["panoptic_seg"][0].cpu(), r["panoptic_seg"][1])} for r in head_results])
    want = on_host.evaluate()
    stats = want["panoptic_seg"]["stats"]
    assert sum(s["tp"] + s["fp"] + s["fn"] for s in stats.values()) > 0
    device_maps = {i: torch.from_numpy(m).to(device) for i, m in id_maps.items()}
    for gt in (PanopticGroundTruth(js, id_maps), PanopticGroundTruth(js, device_maps)):
        ev = COCOPanopticEvaluator(gt, THINGS, STUFF)
        ev.process(inputs, head_results)
        _equal(ev.evaluate(), want)


def test_semantic_fixtures_on_the_device_match_the_reference(device):
    gts, preds, expected = load_fixture()
    ev = SemSegEvaluator(NUM_CLASSES, IGNORE_LABEL, with_pq=True)
    ev.process([{"sem_seg": torch.from_numpy(g).to(device)} for g in gts],
               [{"sem_seg_labels": torch.from_numpy(p.astype(np.int16)).to(device)} for p in preds])
    res = ev.evaluate()["sem_seg"]
    assert stats_rows(res["pq_stats"]) == stats_rows(expected["total"])
    host = SemSegEvaluator(NUM_CLASSES, IGNORE_LABEL, with_pq=True)
    host.process([{"sem_seg": g} for g in gts], [{"sem_seg_labels": p} for p in preds])
    assert np.array_equal(ev.conf_matrix, host.conf_matrix)
    _equal(res, host.evaluate()["sem_seg"])
