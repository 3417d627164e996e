"""Checks of bm2f_amd.image_views that take a device (test_image_views_cpu.py runs them on the CPU definition,
test_image_views_gpu.py on the kernels).  Every comparison is exact equality with what Pillow produced, recorded in
tests/golden/image_views.npz (tests/golden/gen_image_views_golden.py)."""
import functools

import numpy as np
import pytest
import torch
from conftest import golden

import image_view_cases as ivc
from bm2f_amd import DeviceTTAMapper, View, image_views, label_views, preprocess_test_images, resize_image

CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def fixture():
    z = golden("image_views.npz")
    return {k: z[k] for k in z.files}


def view_of(case, source=0):
    return View(size=case["size"], source=source, crop=case["crop"], canvas=case["canvas"], flip_in=case["flip_in"],
                flip_out=case["flip_out"], fill=case["fill"])


def run_image(case, device, **kw):
    src = torch.from_numpy(ivc.image_source(case)).to(device)
    kw.setdefault("out_dtype", torch.uint8)
    out, sizes = image_views([src], [view_of(case)], **kw)
    assert out.device.type == torch.device(device).type and len(sizes) == 1
    return out[0].cpu(), sizes[0]


def image_case(case, device, expected=None):
    got, size = run_image(case, device)
    assert got.dtype == torch.uint8 and tuple(got.shape[1:]) == tuple(size)
    if expected is not None:
        assert np.array_equal(got.numpy(), expected), case["name"]
    assert ivc.matches(fixture(), case["name"], got.numpy()), case["name"]


def run_label(case, device, size_divisibility=0):
    src = torch.from_numpy(ivc.label_source(case)).to(device)
    out, sizes = label_views([src], [view_of(case)], seg_pad=case["seg_pad"], size_divisibility=size_divisibility)
    assert out.dtype == src.dtype and out.shape[:2] == (1, case["planes"])
    return out[0].cpu(), sizes[0]


def label_case(case, device, expected=None):
    got, size = run_label(case, device)
    assert tuple(got.shape[1:]) == tuple(size)
    if expected is not None:
        assert np.array_equal(got.numpy(), expected), case["name"]
    assert ivc.matches(fixture(), case["name"], got.numpy()), case["name"]


def label_batch_pad(device):
    """size_divisibility: the batch pad of label_views is seg_pad too."""
    case = next(c for c in ivc.LABEL_CASES if c["name"] == "lab_uint8_crop_past")
    got, (h, w) = run_label(case, device, size_divisibility=32)
    assert tuple(got.shape[1:]) == (32, 32) and (h, w) == (20, 30)
    assert ivc.matches(fixture(), case["name"], got[:, :h, :w].numpy())
    assert (got[:, h:] == 255).all() and (got[:, :, w:] == 255).all()


def _ragged(device, out_dtype, garbage=False, **kw):
    srcs, big = ivc.ragged_sources()
    bigt = torch.from_numpy(big).to(device)
    y, x = ivc.RAGGED_WINDOW
    h, w = ivc.RAGGED_SOURCES[2]
    tensors = [torch.from_numpy(np.ascontiguousarray(srcs[0])).to(device),
               torch.from_numpy(np.ascontiguousarray(srcs[1])).to(device), bigt[y:y + h, x:x + w]]
    assert not tensors[2].is_contiguous()
    views = [view_of(v, v["source"]) for v in ivc.RAGGED_VIEWS]
    if garbage:
        kw["out"] = torch.full((4, 3, 64, 96), 0xA5, dtype=torch.uint8, device=device).view(out_dtype)
    return tensors, views, image_views(tensors, views, out_dtype=out_dtype, **kw)


def ragged_expected(pad):
    """(V, 3, 64, 96) uint8 from the fixture's canvases: size_divisibility 32 on the largest canvas (40, 67)."""
    fx = fixture()
    exp = np.full((len(ivc.RAGGED_VIEWS), 3, 64, 96), pad, dtype=np.uint8)
    sizes = []
    for i, v in enumerate(ivc.RAGGED_VIEWS):
        c = fx[v["name"]]
        exp[i, :, :c.shape[1], :c.shape[2]] = c
        sizes.append(tuple(c.shape[1:]))
    return exp, sizes


def ragged_batch(device):
    """Every element of (V, 3, Hp, Wp), pads included, in an output pre-filled with garbage."""
    _, _, (out, sizes) = _ragged(device, torch.uint8, garbage=True, size_divisibility=32, pad_value=9)
    exp, esizes = ragged_expected(9)
    assert [tuple(s) for s in sizes] == esizes
    assert tuple(out.shape) == exp.shape
    assert np.array_equal(out.cpu().numpy(), exp)


def output_dtypes(device):
    """fp32 equals torch's (pil.float() - mean) / std bitwise; fp16 and bf16 equal that value .to(dtype); the pad is
    stored as it is; without mean / std a float output holds float(p)."""
    exp, _ = ragged_expected(0)
    mean, std = torch.tensor(ivc.MEAN), torch.tensor(ivc.STD)
    canv = torch.from_numpy(exp)
    want32 = (canv.float() - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    inside = torch.zeros(exp.shape, dtype=torch.bool)
    for i, v in enumerate(ivc.RAGGED_VIEWS):
        h, w = fixture()[v["name"]].shape[1:]
        inside[i, :, :h, :w] = True
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        _, _, (out, _) = _ragged(device, dt, size_divisibility=32, pixel_mean=ivc.MEAN, pixel_std=ivc.STD,
                                 pad_value=-2.5)
        want = torch.where(inside, want32, torch.tensor(-2.5)).to(dt)
        assert out.dtype == dt
        assert torch.equal(out.cpu().view(torch.int16 if dt != torch.float32 else torch.int32),
                           want.view(torch.int16 if dt != torch.float32 else torch.int32)), dt
    _, _, (out, _) = _ragged(device, torch.float32, size_divisibility=32)
    assert torch.equal(out.cpu(), canv.float())


def refusals(device):
    img = torch.zeros(8, 9, 3, dtype=torch.uint8, device=device)
    v = [View(size=(4, 5))]
    with pytest.raises(ValueError, match="uint8"):
        image_views([img.float()], v, out_dtype=torch.float32)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        image_views([torch.zeros(8, 9, 4, dtype=torch.uint8, device=device)], v, out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="65x"):
        image_views([torch.zeros(132, 4, 3, dtype=torch.uint8, device=device)], [View(size=(2, 4))],
                    out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="absent"):
        image_views([img], v, out_dtype=torch.uint8, pixel_mean=ivc.MEAN, pixel_std=ivc.STD)
    with pytest.raises(ValueError, match="empty"):
        image_views([img], [], out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="empty"):
        label_views([torch.zeros(1, 8, 9, dtype=torch.uint8, device=device)], [], seg_pad=255)
    with pytest.raises(ValueError, match="uint8, int16 or int32"):
        label_views([torch.zeros(1, 8, 9, dtype=torch.int64, device=device)], v, seg_pad=0)
    # the limit itself is admitted: 130 -> 2 is 65x, ksize 131
    out, _ = image_views([torch.full((130, 4, 3), 200, dtype=torch.uint8, device=device)], [View(size=(2, 4))],
                         out_dtype=torch.uint8)
    assert (out == 200).all()


def tta_mapper(device):
    from bm2f_amd import SemanticSegmentorWithTTA
    fx = fixture()
    img = torch.from_numpy(ivc.tta_image()).permute(2, 0, 1).contiguous()
    mapper = DeviceTTAMapper(ivc.TTA["min_sizes"], ivc.TTA["max_size"], device=device)
    x = {"image": img, "height": 20, "width": 30}
    views = mapper(x)
    again = mapper(x)
    assert [v["flipped"] for v in views] == [False, True, False, True]
    for i, (v, a) in enumerate(zip(views, again)):
        want = fx[f"tta{i // 2}"]
        want = want[:, :, ::-1] if v["flipped"] else want
        got = v["image"]
        assert got.dtype == torch.uint8 and got.device.type == torch.device(device).type
        assert np.array_equal(got.cpu().numpy(), want), i
        assert torch.equal(got, a["image"])
    # end to end through the TTA wrapper with a stub model: masks from the view's own pixels
    K, Q = 3, 4

    def model(batch):
        (view,) = batch
        im = view["image"].float()
        h, w = im.shape[-2:]
        masks = torch.stack([im[q % 3, ::2, ::2] / 32 - 4 for q in range(Q)])[None]
        logits = torch.eye(Q, K + 1, device=im.device)[None] * 4
        return {"pred_logits": logits, "pred_masks": masks}, (h, w), [(h, w)]

    tta = SemanticSegmentorWithTTA(model, num_classes=K, min_sizes=ivc.TTA["min_sizes"], max_size=ivc.TTA["max_size"],
                                   tta_mapper=mapper)
    (r,) = tta([x])
    assert tuple(r["sem_seg"].shape) == (K, 20, 30) and bool(torch.isfinite(r["sem_seg"]).all())
    assert r["sem_seg"].device.type == torch.device(device).type


def preprocess(device):
    fx = fixture()
    imgs = [torch.from_numpy(a).permute(2, 0, 1).contiguous() for a in ivc.prep_images()]
    batch, sizes = preprocess_test_images([{"image": im} for im in imgs], min_size=ivc.PREP["min_size"],
                                          max_size=ivc.PREP["max_size"], pixel_mean=ivc.MEAN, pixel_std=ivc.STD,
                                          size_divisibility=ivc.PREP["size_divisibility"], device=device)
    assert [tuple(s) for s in sizes] == [(24, 36), (40, 23)]
    mean, std = torch.tensor(ivc.MEAN).view(3, 1, 1), torch.tensor(ivc.STD).view(3, 1, 1)
    want = torch.zeros(2, 3, 64, 64)                          # ImageList.from_tensors: max (40, 36) -> 64, pad 0
    for i in range(2):
        p = torch.from_numpy(fx[f"prep{i}"])
        want[i, :, :p.shape[1], :p.shape[2]] = (p.float() - mean) / std
    assert batch.dtype == torch.float32 and torch.equal(batch.cpu().view(torch.int32), want.view(torch.int32))


def resize_image_is_one_view(device):
    case = ivc.IMAGE_BY_NAME["pair1"]
    got = resize_image(torch.from_numpy(ivc.image_source(case)).to(device), case["size"])
    assert ivc.matches(fixture(), "pair1", got.cpu().numpy())
