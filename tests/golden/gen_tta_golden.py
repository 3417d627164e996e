"""Generate tests/golden/tta.npz by running the REFERENCE's semantic test-time augmentation on the CPU (nothing of the
reference is copied: the fixture holds inputs and results only).

    python tests/golden/gen_tta_golden.py --ref <reference checkout>

``mask2former.test_time_augmentation`` is imported in place with the stand-ins of gen_criterion_golden plus three of
its own: ``fvcore.transforms.HFlipTransform`` (a marker class, which is all the module asks of it),
``detectron2.modeling.DatasetMapperTTA`` and ``detectron2.data.detection_utils.read_image`` (never called: a mapper is
passed and every input carries its image).  The reference's own ``SemanticSegmentorWithTTA._inference_one_image``
(:71-98) then runs with

  * a stand-in mapper that yields the recorded views (each tagged with its index and a transform list that holds an
    HFlipTransform where the view is mirrored), and
  * a stand-in model: the eval branch of MaskFormer.forward (maskformer_model.py:337-364) on that view's recorded
    low-resolution logits -- F.interpolate to the padded size, the reference's ``MaskFormer.semantic_inference``
    (:509-513, called unbound) and a restated ``sem_seg_postprocess`` (crop, then F.interpolate), in either order,

once with ``sem_seg_postprocess_before_inference`` (``before``) and once without (``after``), on one thread as the other
generators do.

Besides the reference's ``sem_seg`` the fixture stores an fp64 evaluation of the same definition per order: the argmax
labels, the runner-up labels and the ambiguity map (top-two margin below 1e-5 relative, the convention of
gen_inference_golden.py).  The generator asserts that at most AMB_CAP of the pixels are ambiguous; the tests assert
the same cap, so the map cannot hide a failure.  If a seed fails the assert, change the seed, not the cap.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

REL = 1e-5        # ambiguity: relative top-two margins below this
AMB_CAP = 0.02    # at most this share of the pixels may be ambiguous

SEED = 7
Q, K = 20, 19                      # a partial query chunk; Cityscapes' class count
OUTPUT = (37, 53)                  # odd width (the flip index), neither side a multiple of the 4 x 32 tile
# (logit (h, w), padded (Hp, Wp), image (Hc, Wc)) per scale; every scale is run plain, then mirrored
SCALES = [((16, 16), (64, 64), (40, 56)), ((24, 32), (96, 128), (75, 106))]


def make_inputs():
    """Per view class logits (Q, K+1) and mask logits (Q, h, w): one smooth scene resized to each view's grid (and
    mirrored for the flipped views, as a model fed the mirrored image would see it) plus per-view noise."""
    g = torch.Generator().manual_seed(SEED)
    scene = F.interpolate(torch.randn(1, Q, 6, 8, generator=g) * 4, size=(48, 64), mode="bilinear",
                          align_corners=False)
    base_cls = torch.randn(Q, K + 1, generator=g)
    base_cls[torch.arange(Q), (torch.arange(Q) * 7) % K] += 5   # every query names a class of its own
    views = []
    for (h, w), padded, image in SCALES:
        for flipped in (False, True):
            m = F.interpolate(scene, size=(h, w), mode="bilinear", align_corners=False)[0]
            if flipped:
                m = m.flip(-1)
            m = m + torch.randn(Q, h, w, generator=g) * 0.5
            cls = base_cls + torch.randn(Q, K + 1, generator=g) * 0.1
            views.append(dict(cls=cls, masks=m.contiguous(), padded=padded, image=image, flipped=flipped))
    return views


def sem_seg_postprocess(result, img_size, output_height, output_width):
    """detectron2.modeling.postprocessing.sem_seg_postprocess: crop to the image, resize to the output."""
    result = result[:, :img_size[0], :img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


def view_sem_seg(semantic_inference, v, before, dtype=torch.float32, output=OUTPUT):
    """One view's sem_seg at the output size (maskformer_model.py:337-364), in `dtype`."""
    cls, masks = v["cls"].to(dtype), v["masks"].to(dtype)
    up = F.interpolate(masks[None], size=v["padded"], mode="bilinear", align_corners=False)[0]
    if before:
        return semantic_inference(cls, sem_seg_postprocess(up, v["image"], *output))
    return sem_seg_postprocess(semantic_inference(cls, up), v["image"], *output)


def fp64_eval(views, before, output=OUTPUT):
    """The same definition in fp64 -> (labels, runner-up labels, ambiguity map, scores); views: dicts with cls,
    masks, padded, image, flipped."""
    def sem(cls, full):
        return torch.einsum("qc,qhw->chw", F.softmax(cls, dim=-1)[..., :-1], full.sigmoid())
    total = 0
    for v in views:
        r = view_sem_seg(sem, v, before, torch.float64, output)
        total = total + (r.flip(dims=[2]) if v["flipped"] else r)
    total = total / len(views)
    top2 = total.topk(2, dim=0)
    amb = (top2.values[0] - top2.values[1]) < REL * top2.values[0]
    return top2.indices[0], top2.indices[1], amb, total


def import_tta(ref_root):
    from gen_criterion_golden import import_reference
    ref = import_reference(ref_root)

    class HFlipTransform:
        pass

    def unavailable(*a, **k):
        raise RuntimeError("stand-in: the generator passes its own mapper and images")

    fv = types.ModuleType("fvcore.transforms")
    fv.HFlipTransform = HFlipTransform
    sys.modules["fvcore.transforms"] = fv
    sys.modules["fvcore"].transforms = fv
    du = types.ModuleType("detectron2.data.detection_utils")
    du.read_image = unavailable
    sys.modules["detectron2.data.detection_utils"] = du
    sys.modules["detectron2.data"].detection_utils = du
    sys.modules["detectron2.data"].__path__ = []
    sys.modules["detectron2.modeling"].DatasetMapperTTA = unavailable
    tta = importlib.import_module("mask2former.test_time_augmentation")
    return ref, tta, HFlipTransform


def run_reference(ref, tta, HFlip, views, before):
    fake = types.SimpleNamespace()
    semantic_inference = lambda cls, full: ref.model.MaskFormer.semantic_inference(fake, cls, full)  # noqa: E731
    calls = []

    def model(batch):
        (x,) = batch
        calls.append(x["view"])
        return [{"sem_seg": view_sem_seg(semantic_inference, views[x["view"]], before)}]

    def mapper(x):
        return [{"view": i, "transforms": types.SimpleNamespace(transforms=[HFlip()] if v["flipped"] else [])}
                for i, v in enumerate(views)]

    seg = tta.SemanticSegmentorWithTTA(types.SimpleNamespace(clone=lambda: None), model, tta_mapper=mapper)
    out = seg._inference_one_image({"height": OUTPUT[0], "width": OUTPUT[1]})
    assert calls == list(range(len(views)))
    return out["sem_seg"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(1)   # one thread: the reference's fp32 reductions do not depend on the host's core count
    from gen_inference_golden import write_npz
    ref, tta, HFlip = import_tta(a.ref)
    views = make_inputs()
    res = {"meta": np.array([Q, K, *OUTPUT, len(views)], dtype=np.int64),
           "geometry": np.array([[*v["masks"].shape[-2:], *v["padded"], *v["image"], int(v["flipped"])] for v in views],
                                dtype=np.int64)}
    for i, v in enumerate(views):
        res[f"view{i}_pred_logits"] = v["cls"].numpy()
        res[f"view{i}_pred_masks"] = v["masks"].numpy()
    npix = OUTPUT[0] * OUTPUT[1]
    for order, before in (("before", True), ("after", False)):
        sem = run_reference(ref, tta, HFlip, views, before)
        assert tuple(sem.shape) == (K, *OUTPUT)
        labels, alt, amb, sem64 = fp64_eval(views, before)
        assert amb.sum().item() <= AMB_CAP * npix, (order, amb.sum().item())
        # the fp32 run and the fp64 evaluation are the same function
        assert (sem.double() - sem64).abs().max() <= 1e-4 * sem64.abs().max(), order
        assert torch.equal(sem.argmax(0)[~amb], labels[~amb]), order
        assert len(labels.unique()) >= 8, (order, "the label map should show many classes")
        res[f"{order}_sem_seg"] = sem.numpy()
        res[f"{order}_labels"] = labels.numpy().astype(np.int16)
        res[f"{order}_alt"] = alt.numpy().astype(np.int16)
        res[f"{order}_amb"] = np.packbits(amb.numpy(), axis=-1)
        print(order, "ambiguous pixels:", int(amb.sum()), "of", npix, "classes present:", len(labels.unique()))
    write_npz(os.path.join(a.out, "tta.npz"), res)
    print("wrote tta.npz")


if __name__ == "__main__":
    main()
