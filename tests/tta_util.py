"""Shared by test_tta_cpu.py and test_tta_gpu.py: the case of tests/golden/tta.npz, synthetic view sets on the same
geometry, and expectations with the ambiguity maps of an fp64 evaluation (gen_tta_golden.fp64_eval).

Bars (inference_util.py): scores within 1e-3 of the expected tensor's max abs value; labels equal to the fp64 argmax
outside the ambiguity map (top-two margin below 1e-5 relative), inside it equal to the argmax or the runner-up.  The
ambiguous share of the pixels is capped at 2 %, as the generator asserts, so the map cannot hide a failure."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
from conftest import golden

import inference_util as iu

AMB_CAP = 0.02
ORDERS = ("before", "after")


@functools.lru_cache(maxsize=None)
def load():
    z = golden("tta.npz")
    Q, K, Ho, Wo, V = (int(v) for v in z["meta"])
    views = []
    for i, (h, w, Hp, Wp, Hc, Wc, flip) in enumerate(z["geometry"].tolist()):
        views.append(dict(cls=torch.from_numpy(z[f"view{i}_pred_logits"]), masks=torch.from_numpy(z[f"view{i}_pred_masks"]),
                          padded=(Hp, Wp), image=(Hc, Wc), flipped=bool(flip)))
        assert tuple(views[-1]["masks"].shape) == (Q, h, w)
    return SimpleNamespace(Q=Q, K=K, output=(Ho, Wo), V=V, views=views)


def expected_fixture(order):
    z = golden("tta.npz")
    Wo = load().output[1]
    return SimpleNamespace(sem_seg=z[f"{order}_sem_seg"], labels=z[f"{order}_labels"], alt=z[f"{order}_alt"],
                           amb=np.unpackbits(z[f"{order}_amb"], axis=-1)[..., :Wo].astype(bool))


def synthetic_views(K, Q, seed=0, geometry=None):
    """Views on the fixture's geometry (or ``geometry``: [(h, w, padded, image, flipped)]) with K classes, Q queries."""
    g = torch.Generator().manual_seed(seed)
    if geometry is None:
        geometry = [(*v["masks"].shape[-2:], v["padded"], v["image"], v["flipped"]) for v in load().views]
    base = torch.randn(Q, K + 1, generator=g)
    base[torch.arange(Q), (torch.arange(Q) * 7) % K] += 5
    return [dict(cls=base + torch.randn(Q, K + 1, generator=g) * 0.1, masks=torch.randn(Q, h, w, generator=g) * 3,
                 padded=padded, image=image, flipped=flipped) for h, w, padded, image, flipped in geometry]


def api_views(views, device=None, dtype=None):
    """The dict form -> the argument of semantic_inference_tta."""
    def put(t, dt=None):
        t = t if dt is None else t.to(dt)
        return t if device is None else t.to(device)
    return [({"pred_logits": put(v["cls"]), "pred_masks": put(v["masks"], dtype)}, v["padded"], v["image"], v["flipped"])
            for v in views]


def expected_from_cpu(views, output, before):
    """The CPU path on the (fp32) views, with the labels and the ambiguity map of an fp64 evaluation."""
    from bm2f_amd import semantic_inference_tta
    from gen_tta_golden import fp64_eval
    K = views[0]["cls"].shape[1] - 1
    sem = semantic_inference_tta(api_views(views), output, num_classes=K, before=before)
    if K == 1:
        zeros = np.zeros(output, dtype=np.int16)
        return SimpleNamespace(sem_seg=sem.numpy(), labels=zeros, alt=zeros, amb=zeros.astype(bool))
    labels, alt, amb, _ = fp64_eval(views, before, output)
    return SimpleNamespace(sem_seg=sem.numpy(), labels=labels.numpy(), alt=alt.numpy(), amb=amb.numpy())


def check(got_scores, got_labels, e, what):
    assert e.amb.sum() <= AMB_CAP * e.amb.size, (what, "too many ambiguous pixels", int(e.amb.sum()))
    if got_scores is not None:
        assert got_scores.dtype == torch.float32
        iu.check_continuous(got_scores, e.sem_seg, what + " sem_seg")
    if got_labels is not None:
        assert got_labels.dtype == torch.int16
        iu.check_discrete(got_labels, e.labels, e.amb, [e.alt], what + " labels")
