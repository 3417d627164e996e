"""Fused inference heads on the GPU: every case of tests/golden/inference.npz x logits in fp32 / fp16 / bf16 through
MaskFormerInference and the compat functions, peak memory of the semantic head, and run-to-run determinism.

fp32 logits are held to the reference's results in the fixture; 16-bit logits to the CPU path on ``logits.float()``
(the definition of correct for them, csrc/resize_device.h).  Bars: inference_util.py."""
import functools

import pytest
import torch

import inference_util as iu

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _expected(name, dt):
    c = iu.load(name)
    if dt == "fp32":
        return [iu.expected_fixture(name, b) for b in range(c.B)]
    return iu.expected_from_cpu(c, c.masks.to(DTYPES[dt]))


def _outputs(c, dt, device):
    return {"pred_logits": c.cls.to(device), "pred_masks": c.masks.to(DTYPES[dt]).to(device)}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", iu.CASES)
def test_module_matches_reference(name, dt, device):
    from bm2f_amd.inference import panoptic_counters
    c = iu.load(name)
    out = _outputs(c, dt, device)
    m = iu.module(c)
    exp = _expected(name, dt)
    res = m(out, c.padded, c.image_sizes, c.output_sizes)
    iu.check_results(res, c, exp)
    assert all(r["sem_seg"].is_cuda and r["panoptic_seg"][0].is_cuda and r["instances"]["pred_masks"].is_cuda
               for r in res)
    iu.check_results(m(out, c.padded, c.image_sizes, c.output_sizes, semantic_labels=True), c, exp, labels=True)
    counters = panoptic_counters(out["pred_logits"], out["pred_masks"], c.padded, c.image_sizes, c.output_sizes,
                                 num_classes=c.K, object_mask_threshold=c.thresholds[0])
    for b in range(c.B):
        iu.check_counters(counters[b], exp[b], f"{name}{b} counters")


def test_semantic_resized_after_inference(device):
    c = iu.load("tiny")
    m = iu.module(c, instance_on=False, panoptic_on=False)
    res = m(_outputs(c, "fp32", device), c.padded, c.image_sizes, c.output_sizes)
    iu.check_continuous(res[0]["sem_seg"], iu.expected_fixture("tiny", 0).sem_seg_after, "sem_seg resized after")


@functools.lru_cache(maxsize=None)
def _compat_expected(name, dt):
    """Per image (full-resolution logits rounded to the tested dtype, expectation): the CPU compat functions on
    exactly those values as fp32, with the ambiguity maps of an fp64 evaluation of the same values."""
    from bm2f_amd import instance_inference, panoptic_inference, semantic_inference
    from bm2f_amd.inference import full_resolution_logits
    c = iu.load(name)
    out = []
    for b in range(c.B):
        full = full_resolution_logits(c.masks[b], c.padded, c.image_sizes[b], c.output_sizes[b]).to(DTYPES[dt])
        f32 = full.float()
        pan, info = panoptic_inference(c.cls[b], f32, num_classes=c.K, thing_classes=range(c.things),
                                       object_mask_threshold=c.thresholds[0], overlap_threshold=c.thresholds[1])
        inst = instance_inference(c.cls[b], f32, num_classes=c.K, test_topk_per_image=c.topk,
                                  thing_classes=range(c.things))
        out.append((full, iu.expected_from_full(c, b, f32, semantic_inference(c.cls[b], f32), pan, info, inst)))
    return out


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", iu.CASES)
def test_compat_functions(name, dt, device):
    """Per-image functions on full-resolution masks (identity geometry), held to the same bars as the module: equal
    outside the ambiguity maps, one of the candidates inside; counters up to the number of ambiguous pixels."""
    from bm2f_amd import instance_inference, panoptic_inference, semantic_inference
    from bm2f_amd.inference import panoptic_counters
    c = iu.load(name)
    for b, (full, e) in enumerate(_compat_expected(name, dt)):
        tag = f"{name}{b} compat"
        cls_d, full_d = c.cls[b].to(device), full.to(device)
        size = tuple(full.shape[-2:])
        iu.check_sem_seg(semantic_inference(cls_d, full_d), e, tag + " sem_seg")
        iu.check_panoptic(panoptic_inference(cls_d, full_d, num_classes=c.K, thing_classes=range(c.things),
                                             object_mask_threshold=c.thresholds[0],
                                             overlap_threshold=c.thresholds[1]), e, tag + " panoptic_seg")
        iu.check_instances(instance_inference(cls_d, full_d, num_classes=c.K, test_topk_per_image=c.topk,
                                              thing_classes=range(c.things)), e, size, tag + " instances")
        counters = panoptic_counters(cls_d[None], full_d[None], size, [size], num_classes=c.K,
                                     object_mask_threshold=c.thresholds[0])
        iu.check_counters(counters[0], e, tag + " counters")
        # labels mode in identity geometry, through the module (the compat functions have no such mode)
        m = iu.module(c, instance_on=False, panoptic_on=False, sem_seg_postprocess_before_inference=True)
        r = m({"pred_logits": cls_d[None], "pred_masks": full_d[None]}, size, [size], semantic_labels=True)
        iu.check_sem_labels(r[0]["sem_seg_labels"], e, tag + " sem_labels")


def test_two_calls_are_bitwise_identical(device):
    c = iu.load("coco")
    out = _outputs(c, "fp32", device)
    m = iu.module(c)
    from bm2f_amd.inference import panoptic_counters
    a = m(out, c.padded, c.image_sizes, c.output_sizes)
    b = m(out, c.padded, c.image_sizes, c.output_sizes)
    la, lb = (m(out, c.padded, c.image_sizes, c.output_sizes, semantic_labels=True) for _ in range(2))
    ca, cb = (panoptic_counters(out["pred_logits"], out["pred_masks"], c.padded, c.image_sizes, c.output_sizes,
                                num_classes=c.K, object_mask_threshold=c.thresholds[0]) for _ in range(2))
    assert sum(len(x) for x in ca) > 0   # the counters built from atomics are really compared
    for x, y in zip(ca, cb):
        assert torch.equal(x, y)
    for ra, rb in zip(la, lb):
        assert torch.equal(ra["sem_seg_labels"], rb["sem_seg_labels"])
    for ra, rb in zip(a, b):
        assert torch.equal(ra["sem_seg"], rb["sem_seg"])
        assert torch.equal(ra["panoptic_seg"][0], rb["panoptic_seg"][0]) and ra["panoptic_seg"][1] == rb["panoptic_seg"][1]
        for k in ("pred_masks", "scores", "pred_classes"):
            assert torch.equal(ra["instances"][k], rb["instances"][k])


def test_semantic_peak_memory(device):
    """coco geometry scaled to logits (64, 64) -> (256, 256): no (Q, Hp, Wp) fp32 intermediate (26 MB) is built."""
    c = iu.load("coco")
    g = torch.Generator().manual_seed(0)
    out = {"pred_logits": torch.randn(1, c.Q, c.K + 1, generator=g).to(device),
           "pred_masks": (torch.randn(1, c.Q, 64, 64, generator=g) * 3).to(device)}
    m = iu.module(c, instance_on=False, panoptic_on=False, sem_seg_postprocess_before_inference=True)
    size = [(256, 256)]
    m(out, size[0], size, size)   # warm-up: library and kernel load
    mb = 1 << 20
    for labels, budget in ((False, None), (True, 16 * mb)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = m(out, size[0], size, size, semantic_labels=labels)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        r = res[0]["sem_seg_labels" if labels else "sem_seg"]
        nbytes = r.numel() * r.element_size()
        print(f"labels={labels}: peak {peak / mb:.2f} MB over the call, result {nbytes / mb:.2f} MB")
        if labels:
            assert r.shape == (256, 256) and peak < budget
        else:
            assert r.shape == (c.K, 256, 256) and peak - nbytes < 16 * mb
        del res, r
