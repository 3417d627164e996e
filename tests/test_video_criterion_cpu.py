"""bm2f_amd.video_criterion on CPU tensors (its plain-torch path) against the reference's own outputs
(tests/golden/video_criterion.npz from tests/golden/gen_video_criterion_golden.py).  No GPU needed.

Bars (the project's, test_criterion_gpu.py:4-6): matched indices exact, losses rtol 1e-5, gradients rtol 1e-4."""
import os

import numpy as np
import pytest
import torch

from bm2f_amd import weaksup
from bm2f_amd.video_criterion import (VideoHungarianMatcherProj, VideoHungarianMatcherProjPair,
                                      VideoSetCriterionProj, VideoSetCriterionProjSpatPair,
                                      VideoSetCriterionProjSpatPairTempPair)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LOSS_ORDER = ("loss_ce", "loss_mask_projection", "loss_mask_spatial_pairwise", "loss_mask_temporal_pairwise")
ALL_LOSSES = ["labels", "projection_masks", "spatial_pairwise", "temporal_pairwise"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "video_criterion.npz"))


def fixture_pairs(z, b):
    """The reference's nested [[(curr (k, 2), next (k, 2))] * (T-1)] * G lists of clip b."""
    G, T = z[f"boxes{b}"].shape[:2]
    p = torch.from_numpy(z[f"pairs{b}"])
    out = []
    for g in range(G):
        per = []
        for t in range(T - 1):
            sel = p[(p[:, 0] == g) & (p[:, 1] == t)]
            per.append((sel[:, 2:4].contiguous(), sel[:, 4:6].contiguous()))
        out.append(per)
    return out


def fixture_targets(z, shared=False):
    """The reference's target dicts (similarity repeated per target, as the reference builds it; ``shared`` ->
    the zero-copy expanded view of the frame's one map)."""
    out = []
    for b in range(int(z["B"])):
        G = z[f"labels{b}"].shape[0]
        sim = torch.from_numpy(z[f"sim{b}"]).float() / float(z["sim_scale"])
        sim = sim[None].expand(G, *sim.shape) if shared else sim[None].repeat(G, 1, 1, 1, 1)
        out.append({"labels": torch.from_numpy(z[f"labels{b}"]),
                    "box_masks": torch.from_numpy(z[f"box_masks{b}"]).float(),
                    "color_similarities": sim, "temporal_pairs": fixture_pairs(z, b)})
    return out


def fixture_heads(z, it):
    n = int(z["n_aux"]) + 1
    return [{"pred_logits": torch.from_numpy(z[f"it{it}_logits{h}"]),
             "pred_masks": torch.from_numpy(z[f"it{it}_masks{h}"]).float() / float(z["mask_scale"])} for h in range(n)]


def fixture_weights(z):
    return dict(zip(LOSS_ORDER, (float(v) for v in z["weights"])))


def build_criterion(z, losses=ALL_LOSSES):
    w = fixture_weights(z)
    warmup = int(z["warmup"])
    matcher = VideoHungarianMatcherProjPair(
        cost_class=w["loss_ce"], cost_projection=w["loss_mask_projection"],
        cost_pairwise=w["loss_mask_spatial_pairwise"], pairwise_size=3, pairwise_dilation=2,
        pairwise_color_thresh=0.3, pairwise_warmup_iters=warmup)
    crit = VideoSetCriterionProjSpatPairTempPair(
        int(z["K"]), matcher=matcher, weight_dict=w, eos_coef=0.1, pairwise_size=3, pairwise_dilation=2,
        pairwise_color_thresh=0.3, pairwise_warmup_iters=warmup, losses=list(losses))
    return matcher, crit


def to_device(targets, device):
    def mv(v):
        if torch.is_tensor(v):
            return v.to(device)
        if isinstance(v, (list, tuple)):
            return type(v)(mv(x) for x in v)
        return v
    return [{k: mv(v) for k, v in t.items()} for t in targets]


def check_against_fixture(z, device, targets, mask_dtype=torch.float32, loss_rtol=1e-5):
    """Run the criterion for the fixture's iterations on `device`; assert indices, losses, gradients, _iter."""
    w = fixture_weights(z)
    n_aux = int(z["n_aux"])
    matcher, crit = build_criterion(z)
    crit = crit.to(device)
    seen = []
    orig = matcher.memory_efficient_forward

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(r)
        return r

    matcher.memory_efficient_forward = spy
    all_losses = []
    for it in range(int(z["iters"])):
        heads = [{"pred_logits": h["pred_logits"].to(device).requires_grad_(),
                  "pred_masks": h["pred_masks"].to(device=device, dtype=mask_dtype).requires_grad_()}
                 for h in fixture_heads(z, it)]
        outputs = dict(heads[-1], aux_outputs=heads[:-1])
        seen.clear()
        losses = crit(outputs, targets)
        assert sorted(losses) == sorted(z["loss_keys"].tolist())
        for call, h in enumerate([n_aux] + list(range(n_aux))):
            for b, (i, j) in enumerate(seen[call]):
                assert np.array_equal(np.stack([i.cpu().numpy(), j.cpu().numpy()]), z[f"it{it}_idx{h}_{b}"]), (it, h, b)
        for k, v in losses.items():
            print(f"it{it} {k}: got {float(v.detach().sum()):.9g} want {float(z[f'it{it}_{k}']):.9g}")
            np.testing.assert_allclose(float(v.detach().sum()), float(z[f"it{it}_{k}"]), rtol=loss_rtol, atol=1e-7, err_msg=k)
        total = sum(v.sum() * w[k.rsplit("_", 1)[0] if k[-1].isdigit() else k] for k, v in losses.items())
        total.backward()
        for h, hd in enumerate(heads):
            np.testing.assert_allclose(hd["pred_logits"].grad.cpu().numpy(), z[f"it{it}_glogits{h}"], rtol=1e-4,
                                       atol=1e-7)
            gm = hd["pred_masks"].grad.float().cpu().numpy()
            if mask_dtype == torch.float32:
                np.testing.assert_allclose(gm, z[f"it{it}_gmasks{h}"], rtol=1e-4, atol=1e-8)
            else:   # the gradient is rounded to the masks' 16-bit type on its way out (fp16: 2^-11 relative)
                np.testing.assert_allclose(gm, z[f"it{it}_gmasks{h}"], rtol=2.0 ** -10, atol=1e-7)
        all_losses.append({k: float(v.detach().sum()) for k, v in losses.items()})
    assert float(crit._iter) == z["iters"] and float(matcher._iter) == z["iters"] * (n_aux + 1)
    return all_losses


@pytest.mark.parametrize("shared", [False, True])
def test_cpu_path_vs_reference(gold, shared):
    check_against_fixture(gold, torch.device("cpu"), fixture_targets(gold, shared=shared))


def test_state_dict_keys_and_loading(gold):
    matcher, crit = build_criterion(gold)
    assert sorted(crit.state_dict().keys()) == sorted(gold["state_keys"].tolist())
    sd = {k: v.clone() for k, v in crit.state_dict().items()}
    sd["_iter"].fill_(7)
    sd["matcher._iter"].fill_(21)
    crit.load_state_dict(sd)
    assert crit._iter_host.peek(crit._iter) == 7.0
    # the reference's VideoHungarianMatcherProj has no buffer; VideoSetCriterionProj has empty_weight and _iter
    proj = VideoSetCriterionProj(5, VideoHungarianMatcherProj(2.0, 5.0), {}, 0.1, ["labels", "projection_masks"])
    assert sorted(proj.state_dict().keys()) == ["_iter", "empty_weight"]


def test_loss_subsets_and_aliases(gold):
    z = gold
    targets = fixture_targets(z)
    heads = fixture_heads(z, 3)
    outputs = dict(heads[-1], aux_outputs=heads[:-1])
    w = fixture_weights(z)
    # every subset gives the full criterion's values for its keys (same matcher, same iteration state)
    _, full = build_criterion(z)
    full._iter.fill_(2)
    full.matcher._iter.fill_(5)
    want = full(outputs, targets)
    for subset in (["labels"], ["projection_masks", "temporal_pairwise"], ["spatial_pairwise"]):
        _, crit = build_criterion(z, subset)
        crit._iter.fill_(2)
        crit.matcher._iter.fill_(5)
        got = crit(outputs, targets)
        assert len(got) == len(subset) * len(heads)
        for k, v in got.items():
            assert torch.equal(v, want[k]), k
    # ProjSpatPair: the same nine-argument constructor
    m = VideoHungarianMatcherProjPair(w["loss_ce"], w["loss_mask_projection"], w["loss_mask_spatial_pairwise"], 3, 2,
                                      0.3, int(z["warmup"]))
    m._iter.fill_(5)
    sp = VideoSetCriterionProjSpatPair(int(z["K"]), m, w, 0.1, 3, 2, 0.3, int(z["warmup"]),
                                       ["labels", "projection_masks", "spatial_pairwise"])
    sp._iter.fill_(2)
    got = sp(outputs, targets)
    for k, v in got.items():
        assert torch.equal(v, want[k]), k
    # Proj: cost_pairwise = 0 reproduces the projection-only matcher
    a = VideoHungarianMatcherProj(2.0, 5.0)
    b = VideoHungarianMatcherProjPair(2.0, 5.0, 0.0)
    bare = [{k: v for k, v in t.items() if k in ("labels", "box_masks")} for t in targets]
    ia, ib = a(heads[0], bare), b(heads[0], targets)
    for (i0, j0), (i1, j1) in zip(ia, ib):
        assert torch.equal(i0, i1) and torch.equal(j0, j1)
    proj = VideoSetCriterionProj(int(z["K"]), a, w, 0.1, ["labels", "projection_masks"])
    got = proj(outputs, bare)
    assert sorted(got) == sorted(k for k in want if k.startswith(("loss_ce", "loss_mask_projection")))
    # the same projection-only matching as scipy on the reference's definition, restated per clip
    from scipy.optimize import linear_sum_assignment
    for bi, t in enumerate(bare):
        x, box = heads[0]["pred_masks"][bi].sigmoid(), t["box_masks"]

        def dice(p, q):
            return 1 - (2 * p @ q.t() + 1) / (p.sum(-1)[:, None] + q.sum(-1)[None] + 1)

        C = -2.0 * heads[0]["pred_logits"][bi].softmax(-1)[:, t["labels"]] + 5.0 * (
            dice(x.amax(3).flatten(1), box.amax(3).flatten(1)) + dice(x.amax(2).flatten(1), box.amax(2).flatten(1)))
        i, j = linear_sum_assignment(C.numpy())
        assert np.array_equal(ia[bi][0].numpy(), i) and np.array_equal(ia[bi][1].numpy(), j)


def test_empty_clip_and_no_targets(gold):
    z = gold
    targets = fixture_targets(z)
    heads = [{k: v.clone().requires_grad_() for k, v in h.items()} for h in fixture_heads(z, 0)]
    T, H, W = (int(z[k]) for k in ("T", "H", "W"))
    empty = {"labels": torch.zeros(0, dtype=torch.int64), "box_masks": torch.zeros(0, T, H, W),
             "color_similarities": torch.zeros(0, T, 8, H, W), "temporal_pairs": []}
    # one clip without targets: the other clip's mask losses are unchanged up to num_masks (4 -> 3 targets)
    _, crit = build_criterion(z)
    crit._iter.fill_(3)
    mixed = crit(dict(heads[-1]), [targets[0], empty])
    for k, v in mixed.items():
        assert torch.isfinite(v).all(), k
    # no targets at all: every mask loss is a zero without gradient, the class loss still trains
    _, crit = build_criterion(z)
    crit._iter.fill_(3)
    losses = crit(dict(heads[-1], aux_outputs=heads[:-1]), [empty, empty])
    for k, v in losses.items():
        if k.startswith("loss_mask"):
            assert not v.requires_grad and float(v.sum()) == 0.0, k
        else:
            assert v.requires_grad and float(v) > 0
    sum(v.sum() for v in losses.values()).backward()
    assert heads[-1]["pred_masks"].grad is None


def test_pack_and_pair_sum_host_logic():
    """Packing: XY -> linear index, endpoint sort, dead pairs; the torch pair sum against the formula."""
    T, H, W = 3, 4, 5
    cur = torch.tensor([[1, 2], [4, 3], [1, 2]], dtype=torch.int32)          # XY; a repeated current pixel
    nxt = torch.tensor([[0, 0], [0, 0], [2, 1]], dtype=torch.int32)          # many-to-one next pixel
    e = torch.zeros((0, 2), dtype=torch.int64)
    clips = [[[(cur, nxt), (e, e)], [(e, e), (e, e)]], [[(e, e), (nxt[:1], cur[:1])]]]
    pk = weaksup.pack_temporal_pairs(clips, T, H, W, torch.device("cpu"))
    assert pk.P == 4 and pk.n_targets == 3 and not bool(pk.bad)
    assert pk.row.tolist() == [0, 0, 0, 2] and pk.t.tolist() == [0, 0, 0, 1]
    assert pk.p0.tolist() == [2 * W + 1, 3 * W + 4, 2 * W + 1, 0] and pk.p1.tolist() == [0, 0, 1 * W + 2, 2 * W + 1]
    assert pk.ep_key.tolist() == sorted(pk.ep_key.tolist())
    # stored order inside a segment: the two pairs that end on next pixel (0, 0) keep their order
    seg = [c for k, c in zip(pk.ep_key.tolist(), pk.ep_code.tolist()) if k == (0 * T + 1) * H * W]
    assert seg == [1, 3]
    g = torch.Generator().manual_seed(0)
    src = (torch.randn(2, T, H, W, generator=g) * 3).requires_grad_()
    rot = torch.tensor([1, -1, 0], dtype=torch.int32)                        # target 1 unmatched
    total, count = weaksup.temporal_pair_sum(src, rot, pk)
    assert int(count) == 4
    x = src.detach().double()
    sig = torch.sigmoid

    def s(a, b):
        return -torch.log(sig(a) * sig(b) + sig(-a) * sig(-b))

    want = s(x[1, 0, 2, 1], x[1, 1, 0, 0]) + s(x[1, 0, 3, 4], x[1, 1, 0, 0]) + s(x[1, 0, 2, 1], x[1, 1, 1, 2]) + \
        s(x[0, 1, 0, 0], x[0, 2, 2, 1])
    np.testing.assert_allclose(float(total), float(want), rtol=1e-6)
    # a coordinate off the frame is flagged and ignored; the criterion raises for it
    bad = [[[(torch.tensor([[5, 0]]), torch.tensor([[0, 0]])), (e, e)]]]
    pk2 = weaksup.pack_temporal_pairs(bad, T, H, W, torch.device("cpu"))
    assert bool(pk2.bad) and pk2.row.tolist() == [-1]
    assert int(weaksup.temporal_pair_sum(src, torch.tensor([0], dtype=torch.int32), pk2)[1]) == 0


def test_bad_pairs_raise(gold):
    z = gold
    targets = fixture_targets(z)
    cur, nxt = targets[1]["temporal_pairs"][0][0]
    broken = cur.clone()
    broken[0, 0] = int(z["W"])
    targets[1]["temporal_pairs"][0][0] = (broken, nxt)
    _, crit = build_criterion(z)
    with pytest.raises(IndexError, match="outside"):
        crit(dict(fixture_heads(z, 0)[-1]), targets)


def test_mining_cpu_vs_reference(gold):
    """weaksup.temporal_pairs on CPU tensors: counts, order and (for unambiguous rows) the reference's choice."""
    check_mining(gold, torch.device("cpu"))


def check_mining(z, device):
    T = int(z["T"])
    err = float(z["cdist_abs_err"])
    rows = single = 0
    for b in range(int(z["B"])):
        feats = torch.from_numpy(z[f"feats{b}"]).float() / float(z["feat_scale"])
        boxes = torch.from_numpy(z[f"boxes{b}"])
        mined = weaksup.temporal_pairs(feats.to(device), boxes.to(device))
        want = fixture_pairs(z, b)
        got = mined.to_lists()
        assert len(got) == len(want) and all(len(g) == T - 1 for g in got)
        for g in range(len(want)):
            for t in range(T - 1):
                wc, wn = want[g][t]
                gc, gn = (v.cpu() for v in got[g][t])
                assert gc.shape == wc.shape and gn.shape == wn.shape, (b, g, t)
                if wc.shape[0] == 0:
                    continue
                assert torch.equal(gc.long(), wc.long()), (b, g, t)            # current pixels: exact, row-major
                x0, y0, x1, y1 = boxes[g, t + 1].tolist()
                assert ((gn[:, 0] >= x0) & (gn[:, 0] < x1) & (gn[:, 1] >= y0) & (gn[:, 1] < y1)).all()
                cx0, cy0, cx1, cy1 = boxes[g, t].tolist()
                a = feats[t, :, cy0:cy1, cx0:cx1].flatten(1).t().double()
                nb = feats[t + 1, :, y0:y1, x0:x1].flatten(1).t().double()
                d = torch.cdist(a, nb, p=2)
                ok = d <= d.amin(1, keepdim=True) * (1 + 2.0 ** -9) + err
                j = (gn[:, 1].long() - y0) * (x1 - x0) + gn[:, 0].long() - x0
                assert ok.gather(1, j[:, None]).all(), (b, g, t)
                one = ok.sum(1) == 1
                assert torch.equal(gn[one].long(), wn[one].long()), (b, g, t)
                rows += d.shape[0]
                single += int(one.sum())
    assert rows > 0 and single >= 0.9 * rows
