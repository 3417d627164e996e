"""bm2f_amd.mask_criterion on CPU tensors (its plain-torch path) against the reference's own outputs
(tests/golden/mask_criterion.npz from tests/golden/gen_mask_criterion_golden.py), with the reference's recorded
random draws replayed through ``point_source``.  No GPU needed.

Bars: matched indices exact; kept (top-k) point sets exact, compared as sets; losses rtol 1e-5; gradients rtol 1e-4 /
atol 1e-6."""
import os

import numpy as np
import pytest
import torch

from bm2f_amd import HungarianMatcher, SetCriterion, VideoHungarianMatcher, VideoSetCriterion

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LOSS_ORDER = ("loss_ce", "loss_mask", "loss_dice")
CASES = ("img", "vid")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "mask_criterion.npz"))


def fixture_targets(z, case, dtype=torch.bool):
    out = []
    for b in range(int(z[f"{case}_B"])):
        w = int(z[f"{case}_size{b}"][1])
        m = torch.from_numpy(np.unpackbits(z[f"{case}_masks{b}"], axis=-1)[..., :w].astype(bool))
        out.append({"labels": torch.from_numpy(z[f"{case}_labels{b}"]), "masks": m.to(dtype)})
    return out


def fixture_heads(z, case):
    return [{"pred_logits": torch.from_numpy(z[f"{case}_logits{h}"]),
             "pred_masks": torch.from_numpy(z[f"{case}_pmasks{h}"]).float() / float(z["mask_scale"])}
            for h in range(int(z["n_aux"]) + 1)]


def fixture_weights(z):
    return dict(zip(LOSS_ORDER, (float(v) for v in z["weights"])))


def build_criterion(z, case, **kw):
    w = fixture_weights(z)
    video = case == "vid"
    matcher = (VideoHungarianMatcher if video else HungarianMatcher)(
        cost_class=w["loss_ce"], cost_mask=w["loss_mask"], cost_dice=w["loss_dice"], num_points=int(z["num_points"]))
    args = dict(matcher=matcher, weight_dict=w, eos_coef=0.1, losses=["labels", "masks"],
                num_points=int(z["num_points"]), oversample_ratio=float(z["oversample"]),
                importance_sample_ratio=float(z["importance"]))
    if not video:
        args["mask_target_type"] = "mask"
    args.update(kw)
    return matcher, (VideoSetCriterion if video else SetCriterion)(int(z["classes"]), **args)


class Replay:
    """point_source that replays the reference's recorded draws: one call per kind per head, in the criterion's head
    order (main, aux 0, aux 1, ...), with the shapes the reference drew."""

    def __init__(self, z, case):
        n_aux = int(z["n_aux"])
        self.z, self.case = z, case
        self.order = [n_aux] + list(range(n_aux))
        self.count = {"match": 0, "oversample": 0, "random": 0}
        self.log = []

    def __call__(self, kind, shape, device):
        head = self.order[self.count[kind]]
        self.count[kind] += 1
        self.log.append(kind)
        v = torch.from_numpy(self.z[f"{self.case}_{kind}{head}"])
        assert tuple(shape) == tuple(v.shape), (kind, head, tuple(shape), tuple(v.shape))
        return v.to(device)


def check_against_fixture(z, case, device, targets, mask_dtype=torch.float32, grad_rtol=1e-4):
    """One criterion call on `device` with the recorded draws; asserts indices, kept sets, losses, gradients."""
    w = fixture_weights(z)
    n_aux = int(z["n_aux"])
    order = [n_aux] + list(range(n_aux))
    matcher, crit = build_criterion(z, case)
    crit = crit.to(device)
    assert crit.point_source is not None and matcher.point_source is None
    crit.point_source = Replay(z, case)
    seen, kept = [], []
    orig_match, orig_sample = matcher.memory_efficient_forward, crit._sample_points

    def spy_match(*a, **k):
        r = orig_match(*a, **k)
        seen.append(r)
        return r

    def spy_sample(*a, **k):
        r = orig_sample(*a, **k)
        kept.append(r)
        return r

    matcher.memory_efficient_forward = spy_match
    crit._sample_points = spy_sample
    heads = [{"pred_logits": h["pred_logits"].to(device).requires_grad_(),
              "pred_masks": h["pred_masks"].to(device=device, dtype=mask_dtype).requires_grad_()}
             for h in fixture_heads(z, case)]
    outputs = dict(heads[-1], aux_outputs=heads[:-1])
    losses = crit(outputs, targets)
    assert sorted(losses) == sorted(z[f"{case}_loss_keys"].tolist())
    assert crit.point_source.log == ["match", "oversample", "random"] * (n_aux + 1)
    n_unc = int(float(z["importance"]) * int(z["num_points"]))
    for call, h in enumerate(order):
        for b, (i, j) in enumerate(seen[call]):
            assert i.dtype == torch.int64 and i.device.type == torch.device(device).type
            assert np.array_equal(np.stack([i.cpu().numpy(), j.cpu().numpy()]), z[f"{case}_idx{h}_{b}"]), (h, b)
        over, want_idx = z[f"{case}_oversample{h}"], z[f"{case}_kept{h}"]
        got = kept[call].cpu().numpy()
        assert got.shape == (over.shape[0], int(z["num_points"]), 2)
        for r in range(over.shape[0]):
            want = {tuple(p) for p in over[r, want_idx[r]].tolist()}
            assert {tuple(p) for p in got[r, :n_unc].tolist()} == want, (h, r)
        assert np.array_equal(got[:, n_unc:], z[f"{case}_random{h}"])
    for k, v in losses.items():
        print(f"{case} {k}: got {float(v.detach().sum()):.9g} want {float(z[f'{case}_{k}']):.9g}")
        np.testing.assert_allclose(float(v.detach().sum()), float(z[f"{case}_{k}"]), rtol=1e-5, atol=0, err_msg=k)
    total = sum(v.sum() * w[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k, v in losses.items())
    total.backward()
    for h, hd in enumerate(heads):
        np.testing.assert_allclose(hd["pred_logits"].grad.cpu().numpy(), z[f"{case}_glogits{h}"], rtol=1e-4, atol=1e-6)
        gm = hd["pred_masks"].grad
        assert gm.dtype == mask_dtype
        np.testing.assert_allclose(gm.float().cpu().numpy(), z[f"{case}_gmasks{h}"], rtol=grad_rtol, atol=1e-6)
    return {k: float(v.detach().sum()) for k, v in losses.items()}


@pytest.mark.parametrize("tdtype", [torch.bool, torch.float32], ids=["bool", "float"])
@pytest.mark.parametrize("case", CASES)
def test_cpu_path_vs_reference(gold, case, tdtype):
    check_against_fixture(gold, case, torch.device("cpu"), fixture_targets(gold, case, tdtype))


@pytest.mark.parametrize("case", CASES)
def test_state_dict_and_repr(gold, case):
    _, crit = build_criterion(gold, case)
    assert sorted(crit.state_dict().keys()) == sorted(gold[f"{case}_state_keys"].tolist())
    assert repr(crit) == str(gold[f"{case}_repr"])
    assert torch.equal(crit.empty_weight, torch.tensor([1.0] * int(gold["classes"]) + [0.1]))


def pool_source(seed=3):
    """A point source whose draws for the first rows do not depend on how many rows are asked for."""
    def source(kind, shape, device):
        g = torch.Generator().manual_seed(seed + {"match": 0, "oversample": 1, "random": 2}[kind])
        return torch.rand((64,) + tuple(shape[1:]), generator=g)[:shape[0]].to(device)
    return source


def check_empty_cases(z, case, device):
    heads = fixture_heads(z, case)
    targets = fixture_targets(z, case)
    B = len(targets)
    to = lambda ts: [{k: v.to(device) for k, v in t.items()} for t in ts]  # noqa: E731

    def run(ts, keep):
        _, crit = build_criterion(z, case)
        crit = crit.to(device)
        crit.point_source = pool_source()
        hs = [{k: v[keep].to(device).requires_grad_() for k, v in h.items()} for h in heads]
        out = crit(dict(hs[-1], aux_outputs=hs[:-1]), to(ts))
        return out, hs

    # no targets at all: zero mask losses that are still connected to pred_masks
    none = [{"labels": t["labels"][:0], "masks": t["masks"][:0]} for t in targets]
    out, hs = run(none, slice(None))
    for k, v in out.items():
        if not k.startswith("loss_ce"):
            assert float(v.detach()) == 0.0, k
    sum(v.sum() for k, v in out.items() if not k.startswith("loss_ce")).backward()
    for h in hs:
        assert h["pred_masks"].grad is not None and not h["pred_masks"].grad.any()
    # an image with G = 0 (the last one): the other images' mask losses are what they are without it, up to num_masks
    # (the same), and its own masks get no gradient
    mixed = targets[:-1] + [none[-1]]
    out, hs = run(mixed, slice(None))
    want, _ = run(targets[:-1], slice(0, B - 1))
    for k in out:
        if not k.startswith("loss_ce"):
            got = float(out[k].detach())
            assert np.isfinite(got) and got > 0
            np.testing.assert_allclose(got, float(want[k].detach()), rtol=1e-5, err_msg=k)
    sum(v.sum() for k, v in out.items() if not k.startswith("loss_ce")).backward()
    for h in hs:
        assert not h["pred_masks"].grad[-1].any() and h["pred_masks"].grad[:-1].any()


@pytest.mark.parametrize("case", CASES)
def test_empty_cases(gold, case):
    check_empty_cases(gold, case, torch.device("cpu"))


def check_box_mask_type(z, device):
    """mask_target_type="box_mask" reads t["box_masks_full"] in the loss (the matcher still reads t["masks"])."""
    heads = fixture_heads(z, "img")
    targets = fixture_targets(z, "img")
    boxed = []
    for t in targets:
        m = t["masks"]
        rows, cols = m.any(2), m.any(1)
        boxed.append(dict(t, box_masks_full=(rows[:, :, None] & cols[:, None, :]).to(device),
                          masks=t["masks"].to(device), labels=t["labels"].to(device)))
    as_masks = [{"labels": t["labels"], "masks": t["box_masks_full"]} for t in boxed]
    out = {k: v.to(device) for k, v in heads[0].items()}
    indices = [(torch.arange(t["labels"].shape[0], device=device), torch.arange(t["labels"].shape[0], device=device))
               for t in boxed]
    res = []
    for kind, ts in (("box_mask", boxed), ("mask", as_masks)):
        _, crit = build_criterion(z, "img", mask_target_type=kind)
        crit.point_source = pool_source()
        res.append(crit.to(device).get_loss("masks", out, ts, indices, 7.0))
    _, crit = build_criterion(z, "img")
    crit.point_source = pool_source()
    other = crit.to(device).get_loss("masks", out, boxed, indices, 7.0)
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
        assert not torch.equal(res[0][k], other[k]), k
    with pytest.raises(ValueError):
        build_criterion(z, "img", mask_target_type="boxes")


def test_box_mask_target_type(gold):
    check_box_mask_type(gold, torch.device("cpu"))


def test_matcher_uses_its_own_source_when_set(gold):
    z = gold
    matcher, crit = build_criterion(z, "img")
    crit.point_source = Replay(z, "img")
    mine = Replay(z, "img")
    matcher.point_source = mine
    h = fixture_heads(z, "img")
    crit(dict(h[-1], aux_outputs=h[:-1]), fixture_targets(z, "img"))
    assert mine.log == ["match"] * 3 and crit.point_source.log == ["oversample", "random"] * 3
    # stand-alone matcher: torch.rand by default, indices on the masks' device, min(Q, G) pairs per image
    matcher.point_source = None
    idx = matcher(h[0], fixture_targets(z, "img"))
    assert [len(i) for i, _ in idx] == [4, 1, 2] and all(i.dtype == torch.int64 for i, _ in idx)
