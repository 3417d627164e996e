"""Semantic test-time augmentation without a GPU: the CPU path of semantic_inference_tta against the reference's
SemanticSegmentorWithTTA (tests/golden/tta.npz), the view sizes, the driver class on stub models and mappers, and the
C entry point's argument checks.  Bars: tta_util.py."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import inference_util as iu
import tta_util as tu


@pytest.mark.parametrize("order", tu.ORDERS)
def test_cpu_path_matches_reference(order):
    from bm2f_amd import semantic_inference_tta
    c = tu.load()
    e = tu.expected_fixture(order)
    kw = dict(num_classes=c.K, before=order == "before")
    sem = semantic_inference_tta(tu.api_views(c.views), c.output, **kw)
    lab = semantic_inference_tta(tu.api_views(c.views), c.output, labels=True, **kw)
    assert tuple(sem.shape) == (c.K, *c.output) and tuple(lab.shape) == c.output
    tu.check(sem, lab, e, f"tta {order}")


def test_fixture_is_a_real_case():
    """The two orders differ by more than twice the bar (an implementation that is within the bar of the wrong order
    is then outside the bar of the right one), flips are present, many classes show."""
    c = tu.load()
    b, a = tu.expected_fixture("before"), tu.expected_fixture("after")
    assert abs(b.sem_seg - a.sem_seg).max() > 2 * iu.RTOL * max(abs(b.sem_seg).max(), abs(a.sem_seg).max())
    assert [v["flipped"] for v in c.views] == [False, True, False, True]
    assert len(set(b.labels.flatten().tolist())) >= 8
    assert c.output[1] % 2 == 1 and c.Q % 32 != 0


def test_view_sizes():
    from bm2f_amd import tta_view_sizes
    sizes = (256, 384, 512, 640, 768, 896)
    views = tta_view_sizes(512, 683, sizes, 3584, True)
    assert len(views) == 12
    assert views[0] == (256, 342, False) and views[1] == (256, 342, True)          # 0.5 * 683 = 341.5 -> 342
    assert views[-2] == (896, 1195, False) and views[-1] == (896, 1195, True)      # 1.75 * 683 = 1195.25
    assert [v[0] for v in views[::2]] == list(sizes) and all(not v[2] for v in views[::2])
    assert all(v[2] for v in views[1::2]) and [v[:2] for v in views[::2]] == [v[:2] for v in views[1::2]]
    # the long side hits max_size: 896 x 8960 scaled by 3584 / 8960 = 0.4 -> 358.4 x 3584
    assert tta_view_sizes(100, 1000, [896], 3584, False) == [(358, 3584, False)]
    # portrait: the width is the short side
    assert tta_view_sizes(683, 512, [256], 3584, False) == [(342, 256, False)]
    assert tta_view_sizes(512, 683, sizes, 3584, False) == views[::2]


@pytest.mark.parametrize("order", tu.ORDERS)
def test_single_view_equals_inference_module(order):
    """V = 1, not mirrored: the mean over one view is MaskFormerInference's sem_seg, bit for bit on the CPU."""
    from bm2f_amd import MaskFormerInference, semantic_inference_tta
    c = tu.load()
    v = c.views[2]
    before = order == "before"
    got = semantic_inference_tta(tu.api_views([v]), c.output, num_classes=c.K, before=before)
    m = MaskFormerInference(num_classes=c.K, sem_seg_postprocess_before_inference=before)
    want = m({"pred_logits": v["cls"][None], "pred_masks": v["masks"][None]}, v["padded"], [v["image"]],
             [c.output])[0]["sem_seg"]
    assert torch.equal(got, want)


def test_rejects_inconsistent_views():
    from bm2f_amd import semantic_inference_tta
    c = tu.load()
    views = tu.api_views(c.views)
    run = lambda vs, K=c.K: semantic_inference_tta(vs, c.output, num_classes=K)   # noqa: E731
    with pytest.raises(ValueError, match="views outside"):
        run([])
    with pytest.raises(ValueError, match="views outside"):
        run(views * 9)
    with pytest.raises(ValueError, match="num_classes"):
        run(views, K=c.K + 1)
    half = tu.api_views(c.views[:1], dtype=torch.float16)
    with pytest.raises(ValueError, match="dtype"):
        run(views[:1] + half)
    other_q = tu.api_views(tu.synthetic_views(c.K, c.Q + 1)[:1])
    with pytest.raises(ValueError, match="queries or classes"):
        run(views[:1] + other_q)
    other_k = tu.api_views(tu.synthetic_views(c.K + 2, c.Q)[:1])
    with pytest.raises(ValueError, match="queries or classes"):
        run(views[:1] + other_k)
    meta = [({"pred_logits": o["pred_logits"], "pred_masks": o["pred_masks"].to("meta")}, p, i, f)
            for o, p, i, f in views[:1]]
    with pytest.raises(ValueError, match="devices"):
        run(views[:1] + meta)


def _stub_model(views, calls):
    """Returns view i's recorded low-resolution outputs for the view dict tagged i, as a batch of one."""
    def model(batch):
        (x,) = batch
        calls.append(x)
        v = views[x["view"]]
        return {"pred_logits": v["cls"][None], "pred_masks": v["masks"][None]}, v["padded"], [v["image"]]
    return model


def _stub_mapper(views, seen):
    def mapper(x):
        seen.append(x)
        return [{"view": i, "image": x["image"], "flipped": v["flipped"]} for i, v in enumerate(views)]
    return mapper


@pytest.mark.parametrize("order", tu.ORDERS)
def test_driver_with_stub_model_and_mapper(order):
    from bm2f_amd import SemanticSegmentorWithTTA
    c = tu.load()
    calls, seen = [], []
    seg = SemanticSegmentorWithTTA(_stub_model(c.views, calls), num_classes=c.K, min_sizes=(40, 75), max_size=200,
                                   before=order == "before", tta_mapper=_stub_mapper(c.views, seen))
    image = torch.zeros(3, 20, 30)
    out = seg([{"image": image, "height": c.output[0], "width": c.output[1]}])
    assert len(out) == 1 and set(out[0]) == {"sem_seg"}
    assert [x["view"] for x in calls] == list(range(c.V))                  # the model ran once per view, in order
    assert all("flipped" not in x and "transforms" not in x for x in calls)
    assert (seen[0]["height"], seen[0]["width"]) == c.output
    tu.check(out[0]["sem_seg"], None, tu.expected_fixture(order), f"driver {order}")   # "height"/"width" honoured
    labels = SemanticSegmentorWithTTA(_stub_model(c.views, []), num_classes=c.K, min_sizes=(40,), max_size=200,
                                      before=order == "before", tta_mapper=_stub_mapper(c.views, []),
                                      semantic_labels=True)([{"image": image, "height": c.output[0],
                                                              "width": c.output[1]}])
    assert set(labels[0]) == {"sem_seg_labels"}
    tu.check(None, labels[0]["sem_seg_labels"], tu.expected_fixture(order), f"driver {order}")


def test_driver_defaults_and_detectron2_style_views():
    """Without "height"/"width" the image's own size is the output; a view marked by an HFlipTransform in its
    "transforms" counts as mirrored; a missing image raises."""
    from bm2f_amd import SemanticSegmentorWithTTA, semantic_inference_tta
    c = tu.load()
    HFlipTransform = type("HFlipTransform", (), {})

    def mapper(x):
        return [{"view": i, "image": x["image"],
                 "transforms": SimpleNamespace(transforms=[HFlipTransform()] if v["flipped"] else [])}
                for i, v in enumerate(c.views)]

    seg = SemanticSegmentorWithTTA(_stub_model(c.views, []), num_classes=c.K, min_sizes=(40,), max_size=200,
                                   tta_mapper=mapper)
    out = seg([{"image": torch.zeros(3, 21, 33)}])[0]["sem_seg"]
    assert torch.equal(out, semantic_inference_tta(tu.api_views(c.views), (21, 33), num_classes=c.K))
    with pytest.raises(ValueError, match="image"):
        seg([{"file_name": "x.png"}])


def test_default_mapper_resizes_and_flips():
    from bm2f_amd import SemanticSegmentorWithTTA, tta_view_sizes
    seen = []

    def model(batch):
        (x,) = batch
        seen.append(x["image"])
        h, w = x["image"].shape[-2:]
        return ({"pred_logits": torch.zeros(1, 4, 4), "pred_masks": torch.zeros(1, 4, (h + 3) // 4, (w + 3) // 4)},
                ((h + 3) // 4 * 4, (w + 3) // 4 * 4), [(h, w)])

    seg = SemanticSegmentorWithTTA(model, num_classes=3, min_sizes=(8, 16), max_size=24, flip=True)
    image = torch.arange(3 * 12 * 20, dtype=torch.float32).view(3, 12, 20)
    out = seg([{"image": image.to(torch.uint8)}, {"image": image}])
    sizes = tta_view_sizes(12, 20, (8, 16), 24, True)
    assert [tuple(i.shape[-2:]) for i in seen[4:]] == [s[:2] for s in sizes] == [(8, 13), (8, 13), (14, 24), (14, 24)]
    assert torch.equal(seen[4].flip(-1), seen[5]) and torch.equal(seen[6].flip(-1), seen[7])
    assert seen[0].is_floating_point()
    assert tuple(out[1]["sem_seg"].shape) == (3, 12, 20)
    # zero logits: every sigmoid is 0.5 and the class probabilities are uniform over K + 1
    assert torch.allclose(out[1]["sem_seg"], torch.full((3, 12, 20), 4 * 0.25 * 0.5))


def test_from_config():
    from bm2f_amd import SemanticSegmentorWithTTA
    cfg = SimpleNamespace(
        TEST=SimpleNamespace(AUG=SimpleNamespace(MIN_SIZES=(256, 384, 512), MAX_SIZE=3584, FLIP=True)),
        MODEL=SimpleNamespace(SEM_SEG_HEAD=SimpleNamespace(NUM_CLASSES=150),
                              MASK_FORMER=SimpleNamespace(TEST=SimpleNamespace(
                                  SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE=True))))
    model = object()
    seg = SemanticSegmentorWithTTA.from_config(cfg, model)
    assert seg.model is model and seg.num_classes == 150 and seg.min_sizes == (256, 384, 512)
    assert seg.max_size == 3584 and seg.flip and seg.before and not seg.semantic_labels
    cfg.TEST.AUG.FLIP = False
    cfg.MODEL.MASK_FORMER.TEST.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE = False
    seg = SemanticSegmentorWithTTA.from_config(cfg, model, semantic_labels=True)
    assert not seg.flip and not seg.before and seg.semantic_labels
    with pytest.raises(ValueError, match="view count"):
        SemanticSegmentorWithTTA(model, num_classes=150, min_sizes=range(100, 117), max_size=3584)


def test_entry_point_rejects_bad_arguments_without_gpu():
    from bm2f_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)

    def tta(lg=p, dtype=0, pr=p, tb=p, v=4, q=100, k=150, o=p, lab=None):
        return lib.m2f_infer_semantic_tta(lg, dtype, 1 << 20, pr, tb, v, q, k, 37, 53, 0, o, lab, None)

    for call in (lambda: tta(lg=None), lambda: tta(pr=None), lambda: tta(tb=None), lambda: tta(o=None)):
        assert call() == 1 and b"null" in lib.m2f_last_error()
    for kw, name in (({"v": 0}, b"num_views"), ({"v": 33}, b"num_views"), ({"k": 257}, b"num_classes"),
                     ({"q": 257}, b"num_queries"), ({"dtype": 7}, b"dtype 7")):
        assert tta(**kw) == 3, kw
        assert name in lib.m2f_last_error() and b"m2f_infer_semantic_tta" in lib.m2f_last_error()
    assert tta(q=0) == 1 and tta(k=0) == 1
    # labels alone is a complete output; a successful call elsewhere clears the thread's message again
    assert tta(o=None, lab=p, v=33) == 3
    assert lib.m2f_masked_attn_plan(1, 1, 64, 8, None, None, None, None) == 0 and lib.m2f_last_error() == b""
