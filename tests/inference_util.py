"""Shared by test_inference_cpu.py and test_inference_gpu.py: the cases of tests/golden/inference.npz, the expected
results (from the fixture, or from the CPU path plus an fp64 evaluation for 16-bit inputs) and the bars.

Bars:
  continuous outputs (sem_seg, instance scores): max abs error <= 1e-3 * the expected tensor's max abs value (the
    project's correctness target, README.md);
  discrete outputs (panoptic_seg, semantic labels, instance pred_masks): equal to the expectation at every pixel
    outside the stored ambiguity map (fp64 margins below 1e-5 relative), inside it equal to one of the candidates;
  segments_info equal as a list; area counters equal up to the number of ambiguous pixels.
Instances are ordered by (class, score): topk(sorted=False) fixes no order and the result does not name its query;
the generator asserts that this order is unambiguous.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
from conftest import golden

CASES = ("coco", "tiny")
RTOL = 1e-3


@functools.lru_cache(maxsize=None)
def load(name):
    z = golden("inference.npz")
    Q, K, things, topk, Hp, Wp = (int(v) for v in z[f"{name}_meta"])
    c = SimpleNamespace(name=name, Q=Q, K=K, things=things, topk=topk, padded=(Hp, Wp),
                        image_sizes=[tuple(int(v) for v in s) for s in z[f"{name}_image_sizes"]],
                        output_sizes=[tuple(int(v) for v in s) for s in z[f"{name}_output_sizes"]],
                        thresholds=tuple(float(v) for v in z[f"{name}_thresholds"]),
                        cls=torch.from_numpy(z[f"{name}_pred_logits"]), masks=torch.from_numpy(z[f"{name}_pred_masks"]))
    c.B = len(c.image_sizes)
    return c


def module(c, **kw):
    from bm2f_amd import MaskFormerInference
    args = dict(num_classes=c.K, thing_classes=range(c.things), semantic_on=True, instance_on=True, panoptic_on=True,
                object_mask_threshold=c.thresholds[0], overlap_threshold=c.thresholds[1],
                test_topk_per_image=c.topk)
    args.update(kw)
    return MaskFormerInference(**args)


def _unpack(a, width):
    return np.unpackbits(a, axis=-1)[..., :width].astype(bool)


@functools.lru_cache(maxsize=None)
def expected_fixture(name, b):
    c = load(name)
    z, key = golden("inference.npz"), f"{name}{b}"
    Wo = c.output_sizes[b][1]
    sem = golden(f"inference_semseg_{key}.npz")
    e = SimpleNamespace(
        sem_seg=sem["sem_seg"], sem_seg_after=sem["sem_seg_after"] if "sem_seg_after" in sem.files else None,
        sem_labels=z[f"{key}_sem_labels"], sem_amb=_unpack(z[f"{key}_sem_amb"], Wo), sem_alt=z[f"{key}_sem_alt"],
        panoptic_seg=z[f"{key}_panoptic_seg"], pan_amb=_unpack(z[f"{key}_pan_amb"], Wo),
        pan_alt=z[f"{key}_pan_alt"], pan_top=z[f"{key}_pan_top"],
        segments_info=[{"id": int(i), "isthing": bool(t), "category_id": int(k)} for i, t, k in z[f"{key}_segments_info"]],
        counters=z[f"{key}_counters"], keep_queries=z[f"{key}_keep_queries"],
        inst_masks=_unpack(z[f"{key}_inst_masks"], Wo), inst_scores=z[f"{key}_inst_scores"],
        inst_classes=z[f"{key}_inst_classes"], inst_queries=z[f"{key}_inst_queries"],
        thr_amb=_unpack(z[f"{key}_thr_amb"], Wo))
    return e


def _assert_separable(scores, classes, what):
    """The (class, score) order pairs instances unambiguously: scores of one class well apart, or exactly zero."""
    o = np.lexsort((scores, classes))
    fin, fcl = np.asarray(scores, dtype=np.float64)[o], np.asarray(classes)[o]
    same = fcl[1:] == fcl[:-1]
    assert np.all(~same | (np.diff(fin) > 1e-4 * fin[1:]) | (fin[1:] == 0)), (what, "instance scores too close")


def expected_from_full(c, b, full, sem, pan, info, inst):
    """Expectation for image b on full-resolution fp32 logits `full` (Q, H, W): the given CPU-path results, with the
    ambiguity maps and candidates of an fp64 evaluation of the same logits."""
    from bm2f_amd import inference as inf
    from gen_inference_golden import fp64_eval, merge_loop
    f = fp64_eval(c.cls[b], full.double(), c.K)
    lut, _, _ = merge_loop(f["classes"].tolist(), f["counters"].tolist(), c.things)
    lut_t = torch.tensor(lut)
    if f["n_keep"]:
        pan_alt, pan_top = lut_t[f["second"] + 1] * f["second_in"], lut_t[f["winner"] + 1]
    else:
        pan_alt = pan_top = f["pan_alt"]
    _, qidx, lab = inf._topk(c.cls[b], c.K, c.topk)
    _assert_separable(inst["scores"].numpy(), inst["pred_classes"].numpy(), f"{c.name}{b}")
    return SimpleNamespace(
        sem_seg=sem.numpy(), sem_seg_after=None, sem_labels=sem.argmax(0).numpy(),
        sem_amb=f["sem_amb"].numpy(), sem_alt=f["sem_alt"].numpy(), panoptic_seg=pan.numpy(),
        pan_amb=f["pan_amb"].numpy(), pan_alt=pan_alt.numpy(), pan_top=pan_top.numpy(), segments_info=info,
        counters=f["counters"].numpy(), keep_queries=f["kidx"].numpy(),
        inst_masks=inst["pred_masks"].numpy() > 0, inst_scores=inst["scores"].numpy(),
        inst_classes=inst["pred_classes"].numpy(), inst_queries=qidx[lab < c.things].numpy(),
        thr_amb=f["thr_amb"].numpy())


def expected_from_cpu(c, masks):
    """Expectation for other inputs (16-bit logits as .float()): the CPU path, with fp64 ambiguity maps."""
    import torch.nn.functional as F
    masks = masks.float()
    res = module(c)({"pred_logits": c.cls, "pred_masks": masks}, c.padded, c.image_sizes, c.output_sizes)
    out = []
    for b, r in enumerate(res):
        up = F.interpolate(masks[b:b + 1].double(), size=c.padded, mode="bilinear", align_corners=False)[0]
        up = up[:, :c.image_sizes[b][0], :c.image_sizes[b][1]]
        if tuple(up.shape[-2:]) != c.output_sizes[b]:
            up = F.interpolate(up[None], size=c.output_sizes[b], mode="bilinear", align_corners=False)[0]
        out.append(expected_from_full(c, b, up, r["sem_seg"], *r["panoptic_seg"], r["instances"]))
    return out


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def check_continuous(got, want, what):
    got, want = _np(got).astype(np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() if got.size else 0.0
    print(f"{what}: max abs err {err:.3e}, bar {RTOL * scale:.3e}")
    assert err <= RTOL * scale, (what, err, scale)


def check_discrete(got, want, amb, candidates, what):
    got, want = _np(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    print(f"{what}: {int(diff.sum())} pixels differ, {int(amb.sum())} ambiguous")
    assert not (diff & ~amb).any(), (what, int((diff & ~amb).sum()))
    ok = ~diff
    for cand in candidates:
        ok |= got == np.asarray(cand).astype(np.int64)
    assert ok.all(), (what, "ambiguous pixel matches no candidate")


def check_sem_seg(got, e, what="sem_seg"):
    check_continuous(got, e.sem_seg, what)


def check_sem_labels(got, e, what="sem_labels"):
    assert got.dtype == torch.int16
    check_discrete(got, e.sem_labels, e.sem_amb, [e.sem_alt], what)


def check_panoptic(got, e, what="panoptic_seg"):
    pan, info = got
    assert pan.dtype == torch.int32
    assert info == e.segments_info, (what, info, e.segments_info)
    check_discrete(pan, e.panoptic_seg, e.pan_amb, [e.pan_alt, e.pan_top, np.zeros_like(e.pan_alt)], what)


def check_counters(got, e, what="counters"):
    got = _np(got).astype(np.int64)
    assert got.shape == e.counters.shape, (what, got.shape, e.counters.shape)
    tol = int(e.pan_amb.sum()) + int(e.thr_amb[e.keep_queries].sum())
    err = np.abs(got - e.counters).max() if got.size else 0
    print(f"{what}: max difference {err}, {tol} ambiguous pixels")
    assert err <= tol, (what, got, e.counters)


def check_instances(got, e, image_size, what="instances"):
    assert set(got) == {"pred_masks", "pred_boxes", "scores", "pred_classes", "image_size"}
    assert tuple(got["image_size"]) == tuple(image_size)
    assert got["pred_masks"].dtype == torch.float32
    assert got["pred_boxes"].shape == (len(e.inst_scores), 4) and not got["pred_boxes"].any()
    gs, gc, gm = _np(got["scores"]), _np(got["pred_classes"]), _np(got["pred_masks"])
    assert gs.shape == e.inst_scores.shape and gm.shape == e.inst_masks.shape, (what, gs.shape, gm.shape)
    og, oe = np.lexsort((gs, gc)), np.lexsort((e.inst_scores, e.inst_classes))
    assert np.array_equal(gc[og], e.inst_classes[oe]), what
    check_continuous(gs[og], e.inst_scores[oe], what + " scores")
    assert np.isin(gm, (0.0, 1.0)).all()
    amb = e.thr_amb[e.inst_queries[oe]]
    diff = (gm[og] > 0) != e.inst_masks[oe]
    print(f"{what} masks: {int(diff.sum())} pixels differ, {int(amb.sum())} ambiguous")
    assert not (diff & ~amb).any(), (what, int((diff & ~amb).sum()))


def check_results(results, c, expected, labels=False):
    """One forward's list of dicts against per-image expectations (all three heads on)."""
    assert len(results) == c.B
    for b, (r, e) in enumerate(zip(results, expected)):
        tag = f"{c.name}{b}"
        if labels:
            assert "sem_seg" not in r
            check_sem_labels(r["sem_seg_labels"], e, tag + " sem_labels")
        else:
            check_sem_seg(r["sem_seg"], e, tag + " sem_seg")
        check_panoptic(r["panoptic_seg"], e, tag + " panoptic_seg")
        check_instances(r["instances"], e, c.output_sizes[b], tag + " instances")
