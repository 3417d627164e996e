"""Inference heads without a GPU: the CPU path of MaskFormerInference and the compat functions against the
reference's results (tests/golden/inference.npz), from_config's or-rule, and the C entry points' argument checks."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import inference_util as iu


@pytest.mark.parametrize("name", iu.CASES)
def test_module_cpu_matches_reference(name):
    c = iu.load(name)
    res = iu.module(c)({"pred_logits": c.cls, "pred_masks": c.masks}, c.padded, c.image_sizes, c.output_sizes)
    iu.check_results(res, c, [iu.expected_fixture(name, b) for b in range(c.B)])


@pytest.mark.parametrize("name", iu.CASES)
def test_module_cpu_labels_and_counters(name):
    from bm2f_amd.inference import panoptic_counters
    c = iu.load(name)
    exp = [iu.expected_fixture(name, b) for b in range(c.B)]
    res = iu.module(c)({"pred_logits": c.cls, "pred_masks": c.masks}, c.padded, c.image_sizes, c.output_sizes,
                       semantic_labels=True)
    iu.check_results(res, c, exp, labels=True)
    counters = panoptic_counters(c.cls, c.masks, c.padded, c.image_sizes, c.output_sizes, num_classes=c.K,
                                 object_mask_threshold=c.thresholds[0])
    for b in range(c.B):
        iu.check_counters(counters[b], exp[b], f"{name}{b} counters")


def test_fixture_reaches_every_panoptic_event():
    """An image without any kept query (zeros map, empty list), merged stuff segments and an original_area of 0."""
    e = iu.expected_fixture("coco", 1)
    assert e.segments_info == [] and not e.panoptic_seg.any() and len(e.counters) == 0
    for name in iu.CASES:
        e = iu.expected_fixture(name, 0)
        assert (e.counters[:, 1] == 0).any()
        assert len(e.segments_info) < len(e.counters)


def test_semantic_resized_after_inference():
    """sem_seg_postprocess_before_inference = False: the scores are resized, not the logits (:362-364)."""
    c = iu.load("tiny")
    m = iu.module(c, instance_on=False, panoptic_on=False)
    assert not m.sem_seg_postprocess_before_inference
    res = m({"pred_logits": c.cls, "pred_masks": c.masks}, c.padded, c.image_sizes, c.output_sizes)
    assert set(res[0]) == {"sem_seg"}
    iu.check_continuous(res[0]["sem_seg"], iu.expected_fixture("tiny", 0).sem_seg_after, "sem_seg resized after")
    with pytest.raises(ValueError):
        m({"pred_logits": c.cls, "pred_masks": c.masks}, c.padded, c.image_sizes, c.output_sizes, semantic_labels=True)


@pytest.mark.parametrize("name", iu.CASES)
def test_compat_functions_cpu(name):
    """The reference's per-image functions on full-resolution masks."""
    from bm2f_amd import instance_inference, panoptic_inference, semantic_inference
    from bm2f_amd.inference import full_resolution_logits
    c = iu.load(name)
    for b in range(c.B):
        e = iu.expected_fixture(name, b)
        full = full_resolution_logits(c.masks[b], c.padded, c.image_sizes[b], c.output_sizes[b])
        iu.check_sem_seg(semantic_inference(c.cls[b], full), e)
        iu.check_panoptic(panoptic_inference(c.cls[b], full, num_classes=c.K, thing_classes=range(c.things),
                                             object_mask_threshold=c.thresholds[0],
                                             overlap_threshold=c.thresholds[1]), e)
        iu.check_instances(instance_inference(c.cls[b], full, num_classes=c.K, test_topk_per_image=c.topk,
                                              thing_classes=range(c.things)), e, c.output_sizes[b])
        every = instance_inference(c.cls[b], full, num_classes=c.K, test_topk_per_image=c.topk)
        assert every["scores"].shape == (c.topk,) and every["pred_masks"].shape == (c.topk, *c.output_sizes[b])


def _cfg(sem, inst, pan, before):
    test = SimpleNamespace(SEMANTIC_ON=sem, INSTANCE_ON=inst, PANOPTIC_ON=pan, OBJECT_MASK_THRESHOLD=0.7,
                           OVERLAP_THRESHOLD=0.6, SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE=before)
    return SimpleNamespace(MODEL=SimpleNamespace(MASK_FORMER=SimpleNamespace(TEST=test),
                                                 SEM_SEG_HEAD=SimpleNamespace(NUM_CLASSES=19)),
                           TEST=SimpleNamespace(DETECTIONS_PER_IMAGE=50))


@pytest.mark.parametrize("inst,pan,before", [(a, b, c) for a in (False, True) for b in (False, True)
                                             for c in (False, True)])
def test_from_config_or_rule(inst, pan, before):
    from bm2f_amd import MaskFormerInference
    meta = SimpleNamespace(thing_dataset_id_to_contiguous_id={11: 3, 12: 4})
    m = MaskFormerInference.from_config(_cfg(True, inst, pan, before), meta)
    assert m.sem_seg_postprocess_before_inference == (before or pan or inst)   # maskformer_model.py:237-241
    assert (m.semantic_on, m.instance_on, m.panoptic_on) == (True, inst, pan)
    assert (m.num_classes, m.test_topk_per_image, m.thing_classes) == (19, 50, (3, 4))
    assert (m.object_mask_threshold, m.overlap_threshold) == (0.7, 0.6)


def test_entry_points_reject_bad_arguments_without_gpu():
    from bm2f_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    geo = (8, 12, 32, 48, 32, 48)   # in_h, in_w, pad_h, pad_w, out_h, out_w
    sem = lambda lg=p, pr=p, sz=p, q=100, k=133, o=p: lib.m2f_infer_semantic(lg, 0, pr, sz, 1, q, k, *geo, o, None, None)
    pan = lambda lg=p, q=100, w=p: lib.m2f_infer_panoptic_pass(lg, 0, p, p, p, p, 1, q, *geo, w, p, p, None)
    ins = lambda lg=p, q=100, tiles=2, m=p: lib.m2f_infer_instance(lg, 0, p, p, p, 1, q, 10, *geo, tiles, m, p, p, None)
    for call in (lambda: sem(lg=None), lambda: sem(pr=None), lambda: sem(sz=None), lambda: sem(o=None),
                 lambda: pan(lg=None), lambda: pan(w=None), lambda: ins(lg=None), lambda: ins(m=None)):
        assert call() == 1 and b"null" in lib.m2f_last_error()
    assert sem(k=257) == 3 and b"num_classes" in lib.m2f_last_error()
    for call in (lambda: sem(q=257), lambda: pan(q=257), lambda: ins(q=257)):
        assert call() == 3 and b"num_queries" in lib.m2f_last_error()
    assert ins(tiles=3) == 1 and b"num_tiles" in lib.m2f_last_error()
    # the fp32 pixel count of a mask is exact only up to 2^24 pixels
    assert lib.m2f_infer_instance(p, 0, p, p, p, 1, 100, 10, 8, 12, 32, 48, 8192, 4096, 32768, p, p, p, None) == 3
    assert lib.m2f_infer_semantic(p, 7, p, p, 1, 100, 133, *geo, p, None, None) == 3
    # a successful call clears the thread's message again (other tests expect a clean slate)
    assert lib.m2f_masked_attn_plan(1, 1, 64, 8, None, None, None, None) == 0 and lib.m2f_last_error() == b""


def test_cpu_path_accepts_16bit_logits_as_float():
    c = iu.load("tiny")
    m = iu.module(c)
    args = (c.padded, c.image_sizes, c.output_sizes)
    half = c.masks.half()
    a = m({"pred_logits": c.cls, "pred_masks": half}, *args)[0]
    b = m({"pred_logits": c.cls, "pred_masks": half.float()}, *args)[0]
    assert torch.equal(a["sem_seg"], b["sem_seg"]) and torch.equal(a["panoptic_seg"][0], b["panoptic_seg"][0])
