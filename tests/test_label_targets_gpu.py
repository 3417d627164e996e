"""Label-map training targets on the device: the helpers and the label histogram (csrc/label_counts.hip), and the
label-map entry points of csrc/point_sample.hip against the dense path given ``label_targets_to_masks`` of the same
targets.

Bars: everything that is reduced in a fixed order (the match cost, the four forward sums of the loss, hence the
mask losses of the criterion; ``loss_ce`` is torch's own atomically reduced op, see ``cases.same_loss``) is bitwise
equal to the dense uint8 path: a tap's value is exactly 0 or 1 either way and the
taps are summed in the same order.  The loss gradient scatters with fp32 atomics and is not ordered; it is held to
test_mask_criterion_gpu.py's own bar against the fp64 restatement (twice fp32 ``grid_sample``'s error, floor 1e-6 of
the maximum).  For fp16 logits that bar is put to the kernel's fp32 gradient buffer; the autograd wrapper's rounding
of it to fp16 is the dense path's own and is covered by the criterion test (rtol 2^-10)."""
import pytest
import torch
import torch.nn.functional as F

import label_target_cases as cases
import test_mask_criterion_gpu as dense_tests
from bm2f_amd import _native, label_counts, label_targets_to_masks
from bm2f_amd import mask_criterion as mc

pytestmark = pytest.mark.gpu

DTYPE_IDS = [str(d).replace("torch.", "") for d in cases.MAP_DTYPES]


# ------------------------------------------------------------------------------------------------------------
# helpers and histogram
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.MAP_DTYPES, ids=DTYPE_IDS)
def test_semantic_targets(device, dtype):
    cases.check_semantic_targets(device, dtype)


@pytest.mark.parametrize("dtype", cases.MAP_DTYPES, ids=DTYPE_IDS)
def test_panoptic_targets(device, dtype):
    cases.check_panoptic_targets(device, dtype)


@pytest.mark.parametrize("bins", [19, 150, "beyond_lds"])
@pytest.mark.parametrize("dtype", cases.MAP_DTYPES[:3], ids=DTYPE_IDS[:3])
def test_label_histogram(device, dtype, bins):
    """19 and 150 bins: the LDS path (and the global one, forced); beyond the LDS capacity: the global path."""
    if bins == "beyond_lds":
        bins = label_counts.geometry()[2] + 5
    cases.check_histogram(device, dtype, bins)


# ------------------------------------------------------------------------------------------------------------
# match cost, kernel alone
# ------------------------------------------------------------------------------------------------------------
def _label_targets(g, sizes, Gs, dtype, ignore_share=0.2):
    """Random per-pixel label maps with G ids each (the first id of an image with G > 2 has no pixels) plus pixels
    of a value that is no id."""
    top = 200 if dtype == torch.uint8 else 30000
    out = []
    for (h, w), G in zip(sizes, Gs):
        ids = torch.randperm(top, generator=g)[:G + 2] + 1
        void, unused, ids = int(ids[0]), int(ids[1]), ids[2:]
        pool = ids[1:] if G > 2 else ids
        m = pool[torch.randint(len(pool), (h, w), generator=g)] if G else torch.full((h, w), unused)
        m[torch.rand(h, w, generator=g) < ignore_share] = void
        out.append({"labels": torch.zeros(G, dtype=torch.int64), "label_map": m.to(dtype), "ids": ids.to(torch.int32)})
    return out


# every shape of the dense kernel's test as an image batch (its T = 0 shapes, and the T = 3 ones without their frames)
IMAGE_SHAPES = [s[:5] for s in dense_tests.MATCH_SHAPES]


@pytest.mark.parametrize("dtype", cases.MAP_DTYPES[:3], ids=DTYPE_IDS[:3])
@pytest.mark.parametrize("shape", IMAGE_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_match_cost_labels_vs_dense(device, shape, dtype):
    H, W, K, Q, Gs = shape
    g = torch.Generator().manual_seed(H * 1000 + K)
    B, Gm = len(Gs), max(Gs)
    masks = (torch.randn(B, Q, H, W, generator=g) * 4).to(device)
    coords = dense_tests._coords(g, B, K, H, W).to(device)
    cls = -torch.rand(B, Q, Gm, generator=g).to(device)
    weights = (2.0, 5.0, 3.0)
    targets = [{k: v.to(device) for k, v in t.items()} for t in _label_targets(g, [(4 * H, 4 * W)] * B, Gs, dtype)]
    tl = mc.MaskTargets(targets, device, False)
    td = mc.MaskTargets([{"labels": t["labels"], "masks": label_targets_to_masks(t)} for t in targets], device, False)
    pl, pd = tl.planes("masks"), td.planes("masks")
    assert pl["code"] == 2 and pd["code"] == 0 and pl["label_bytes"] == targets[0]["label_map"].element_size()
    assert pl["list"][0].data_ptr() == targets[0]["label_map"].data_ptr()          # read in place
    got = mc.match_cost(masks, coords, pl["match"], 2, Gm, cls, *weights, label_bytes=pl["label_bytes"])
    again = mc.match_cost(masks, coords, pl["match"], 2, Gm, cls, *weights, label_bytes=pl["label_bytes"])
    want = mc.match_cost(masks, coords, pd["match"], 0, Gm, cls, *weights)
    assert torch.equal(got, again)
    assert torch.equal(got, want)
    assert want.abs().sum() > 0
    for b, G in enumerate(Gs):
        assert not got[b, :, G:].any()


# ------------------------------------------------------------------------------------------------------------
# loss sums and gradient
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dtype", cases.MAP_DTYPES[:3], ids=DTYPE_IDS[:3])
@pytest.mark.parametrize("hwk", [(7, 5, 130), (20, 28, 1100)], ids=lambda s: "x".join(map(str, s)))
def test_loss_rows_labels_vs_dense(device, hwk, dtype, mdtype):
    """Two images of different sizes, coordinates normalised over the batch's padded size ((Hn, Wn) != (Ht, Wt) for
    the second); one row's id has no pixels.  K = 1100: two chunks of the forward's partials."""
    H, W, K = hwk
    g = torch.Generator().manual_seed(H + K)
    masks = (torch.randn(3, 4, H, W, generator=g) * 4).to(mdtype)
    plane = torch.tensor([7, 0, 11, 7, 2], dtype=torch.int64)
    sizes = [(4 * H, 4 * W), (3 * H, 3 * W + 1)]
    Hn, Wn = 4 * H, 4 * W
    tg = [{k: v.to(device) for k, v in t.items()} for t in _label_targets(g, sizes, [4, 3], dtype)]
    row_of = [(0, 1), (0, 3), (1, 2), (1, 0), (0, 1)]                  # (image, target); (1, 0) has no pixels
    assert not label_targets_to_masks(tg[1])[0].any() and label_targets_to_masks(tg[1])[2].any()
    R = len(row_of)
    coords = dense_tests._coords(g, R, K, H, W)
    dense = [label_targets_to_masks(tg[b])[j].view(torch.uint8).contiguous() for b, j in row_of]
    rows_l = torch.tensor([[tg[b]["label_map"].data_ptr(), int(tg[b]["ids"][j]), *sizes[b], Hn, Wn] for b, j in row_of],
                          dtype=torch.int64).to(device)
    rows_d = torch.tensor([[d.data_ptr(), *sizes[b], Hn, Wn] for d, (b, _) in zip(dense, row_of)],
                          dtype=torch.int64).to(device)
    item = tg[0]["label_map"].element_size()
    md, pd, cd = masks.to(device), plane.to(device), coords.to(device)
    got = mc.point_loss_sums(md, pd, cd, rows_l, 2, keep=tg, label_bytes=item)
    want = mc.point_loss_sums(md, pd, cd, rows_d, 0, keep=dense)
    for name, a, b in zip(("bce", "sum sig t", "sum sig", "sum t"), got, want):
        assert torch.equal(a, b), name
    assert float(got[3][3]) == 0.0 and float(got[3][0]) > 0                 # the row without pixels: sum t = 0
    # the gradient kernel's fp32 buffer against the fp64 restatement on the zero-padded dense targets
    padded = torch.stack([F.pad(d.cpu().float(), (0, Wn - d.shape[1], 0, Hn - d.shape[0])) for d in dense])
    grads = [torch.randn(R, generator=g) for _ in range(3)]
    m32 = masks.float()
    s32, _, g32 = dense_tests._rows_ref(m32, plane, coords, padded, torch.float32, grads)
    s64, _, g64 = dense_tests._rows_ref(m32, plane, coords, padded, torch.float64, grads)
    for name, a, lo, hi in zip(("bce", "sum sig t", "sum sig", "sum t"), got, s32, s64):
        dense_tests._check(name, a, lo, hi)
    grad = torch.zeros(masks.shape, dtype=torch.float32, device=device)
    gr = torch.stack(grads, 1).contiguous().to(device)
    _native.call("m2f_point_loss_bwd_labels", md.data_ptr(), _native.dtype_code(mdtype, "test"), 12, H, W, pd.data_ptr(), R,
                 cd.data_ptr(), K, rows_l.data_ptr(), item, gr.data_ptr(), grad.data_ptr(), _native.stream(md))
    dense_tests._check("grad", grad, g32, g64)
    assert not grad.cpu()[g64 == 0].any()                                    # untouched pixels stay exactly zero
    if mdtype == torch.float32:                                              # and through autograd
        mg = md.clone().requires_grad_()
        out = mc.point_loss_sums(mg, pd, cd, rows_l, 2, keep=tg, label_bytes=item)
        sum((o * x.to(device)).sum() for o, x in zip(out[:3], grads)).backward()
        dense_tests._check("autograd grad", mg.grad, g32, g64)


def test_label_entry_points_refuse_unknown_widths(device):
    x = torch.zeros(1, 1, 4, 4, device=device)
    t = torch.zeros(1, 6, dtype=torch.int64, device=device)
    with pytest.raises(_native.NativeError, match="bytes per label"):
        mc.point_loss_sums(x, torch.zeros(1, dtype=torch.int64, device=device), torch.zeros(1, 3, 2, device=device), t, 2,
                           label_bytes=8)


# ------------------------------------------------------------------------------------------------------------
# whole criterion and matcher
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64], ids=["uint8", "int32", "int64"])
def test_criterion_label_maps_vs_dense(device, dtype, mdtype):
    cases.check_criterion(device, bitwise=True, map_dtype=dtype, mask_dtype=mdtype)


def test_empty_cases_and_errors(device):
    cases.check_empty_and_errors(device, bitwise=True)


# ------------------------------------------------------------------------------------------------------------
# no dense planes
# ------------------------------------------------------------------------------------------------------------
def test_no_dense_planes_are_allocated(device):
    """4 maps of 256 x 256 with 30 ids each, Q = 40: the peak of a criterion call above what is allocated before it
    stays below the bytes of the dense bool planes alone plus the peak of the same call on 8 x 8 maps."""
    B, G, Q = 4, 30, 40
    g = torch.Generator().manual_seed(8)
    heads = [{"pred_logits": torch.randn(B, Q, cases.NUM_CLASSES + 1, generator=g).to(device),
              "pred_masks": torch.randn(B, Q, 32, 32, generator=g).to(device)} for _ in range(3)]
    outputs = dict(heads[-1], aux_outputs=heads[:-1])

    def peak(size):
        maps = [torch.randint(1, G + 1, (size, size), generator=g).to(torch.int32).to(device) for _ in range(B)]
        infos = [[{"id": i + 1, "category_id": i % cases.NUM_CLASSES, "iscrowd": 0} for i in range(G)]] * B
        targets = cases.panoptic_targets(maps, infos)
        _, crit = cases.build(num_points=112)
        crit.point_source = mc._rand_source                                  # 120 matched rows: beyond the pool's 64
        crit = crit.to(device)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(device)
        before = torch.cuda.memory_allocated(device)
        losses = crit(outputs, targets)
        torch.cuda.synchronize()
        assert all(torch.isfinite(v) for v in losses.values())
        return torch.cuda.max_memory_allocated(device) - before

    peak(8)                                                                  # warm-up: code objects, workspaces
    small, large = peak(8), peak(256)
    planes = B * G * 256 * 256
    print(f"peak above the call's start: 8 x 8 maps {small} B, 256 x 256 maps {large} B; dense bool planes {planes} B")
    assert large < planes + small
