"""Video inference (bm2f_amd/video_inference.py) and clip target preparation (bm2f_amd/video_targets.py) on CPU
tensors against the reference's results in tests/golden/video_model.npz, and the C-ABI argument checks of the two
entry points (no GPU needed).  The helpers are shared with test_video_model_gpu.py.

Bars.  Inference: (label, score) sets equal, scores rtol 1e-6; masks equal outside the fixture's ambiguity map (an
fp64 |logit| below 1e-5 of its mask's maximum); the packed form equals the bool form, tail bits zero.  Targets:
labels, ids, masks, box rasters and bounds exact; Lab rtol 1e-6 / atol 1e-5 and colour similarity rtol 1e-5 / atol
1e-6 (the bars of test_target_prep_vs_reference); resized features bitwise (the fixture's features are multiples of
1/16 and the stride-4 weights are 1/2: exact in fp32); mined pairs under the admissibility rule of
test_mining_vs_reference; the pair counters within the number of ambiguous rows."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from bm2f_amd import (VideoMaskFormerInference, feat_resize_pad, pack_mask_bits, prepare_video_targets,
                      prepare_video_weaksup_targets, unpack_mask_bits)
from bm2f_amd import video_targets as vt
from bm2f_amd import weaksup

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ("a", "b", "c", "d")
CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(GOLD, "video_model.npz"))


# -------------------------------------------------------------------------------------------------------------------
# inference helpers
# -------------------------------------------------------------------------------------------------------------------
def infer_case(name, device=CPU, dtype=torch.float32):
    """-> (module, outputs, padded, image, output) of a fixture case; the logits are exact in fp16 and bf16."""
    z = gold()
    Q, K, T, topk, scale = (int(v) for v in z["infer_meta"])
    g = [int(v) for v in z[f"{name}_geometry"]]
    masks = (torch.from_numpy(z[f"{name}_pred_masks"]).float() / scale).to(dtype)
    out = {"pred_logits": torch.from_numpy(z[f"{name}_pred_logits"])[None].to(device),
           "pred_masks": masks[None].to(device)}
    return VideoMaskFormerInference(K, topk), out, tuple(g[0:2]), tuple(g[2:4]), tuple(g[4:6])


def _order(labels, scores):
    return np.lexsort((np.asarray(scores, dtype=np.float64), np.asarray(labels)))


def check_inference(res, name):
    """The module's dict against the reference's: entries paired by (label, score)."""
    z = gold()
    Ho, Wo = (int(v) for v in z[f"{name}_geometry"][4:6])
    assert tuple(res["image_size"]) == (Ho, Wo)
    want_l, want_s = z[f"{name}_labels"], z[f"{name}_scores"]
    assert len(res["pred_scores"]) == len(res["pred_labels"]) == len(res["pred_masks"]) == len(want_l)
    assert all(isinstance(v, float) for v in res["pred_scores"]) and all(isinstance(v, int) for v in res["pred_labels"])
    og, ow = _order(res["pred_labels"], res["pred_scores"]), _order(want_l, want_s)
    assert np.array_equal(np.asarray(res["pred_labels"])[og], want_l[ow])
    np.testing.assert_allclose(np.asarray(res["pred_scores"])[og], want_s[ow], rtol=1e-6)
    want_m = np.unpackbits(z[f"{name}_masks"], axis=-1)[..., :Wo].astype(bool)
    amb = np.unpackbits(z[f"{name}_amb"], axis=-1)[..., :Wo].astype(bool)
    for i, j in zip(og, ow):
        m = res["pred_masks"][i]
        assert m.dtype == torch.bool and m.device.type == "cpu" and tuple(m.shape) == want_m[j].shape
        bad = (m.numpy() != want_m[j]) & ~amb[j]
        assert not bad.any(), f"case {name} entry {i}: {int(bad.sum())} pixels differ outside the ambiguity map"


def check_packed(res_packed, res, width):
    """The packed dict holds the same entries in the same order; bits equal the bool form, tail bits zero."""
    assert res_packed["packed"] is True and "packed" not in res
    assert res_packed["pred_scores"] == res["pred_scores"] and res_packed["pred_labels"] == res["pred_labels"]
    assert tuple(res_packed["image_size"]) == tuple(res["image_size"])
    for words, m in zip(res_packed["pred_masks"], res["pred_masks"]):
        assert words.dtype == torch.int32 and words.device.type == "cpu"
        assert tuple(words.shape) == (*m.shape[:-1], (width + 31) // 32)
        assert torch.equal(words, pack_mask_bits(m))            # pack zero-fills the tail
        assert torch.equal(unpack_mask_bits(words, width), m)


# -------------------------------------------------------------------------------------------------------------------
# target helpers
# -------------------------------------------------------------------------------------------------------------------
class _Tensor:
    def __init__(self, tensor):
        self.tensor = tensor


class _Instances:
    """The fields of a detectron2 Instances that the target preparation reads."""

    def __init__(self, d):
        self.image_size = d["image_size"]
        self.gt_boxes, self.gt_masks = _Tensor(d["boxes"]), _Tensor(d["masks"])
        self.gt_classes, self.gt_ids = d["labels"], d["ids"]


def clip_inputs(device=CPU, as_instances=False, feat_dtype=torch.float32):
    """-> (targets, org_images, org_dino_feats) of the fixture's clips."""
    z = gold()
    B, T, D, Hp, Wp, scale = (int(v) for v in z["target_meta"])
    targets, images, feats = [], [], []
    for b in range(B):
        boxes = torch.from_numpy(z[f"boxes{b}"])
        ids = torch.from_numpy(z[f"in_ids{b}"])
        Hf, Wf = z[f"image{b}_0"].shape[-2:]
        masks = torch.from_numpy(np.unpackbits(z[f"in_masks{b}"], axis=-1)[..., :Wf].astype(bool))   # (G, T, Hf, Wf)
        frames = [{"boxes": boxes[:, t].to(device), "labels": torch.from_numpy(z[f"in_labels{b}"]).to(device),
                   "ids": ids[:, t].to(device), "masks": masks[:, t].to(device), "image_size": (Hf, Wf)}
                  for t in range(T)]
        targets.append({"instances": [_Instances(f) for f in frames]} if as_instances else frames)
        images += [torch.from_numpy(z[f"image{b}_{t}"]).to(device) for t in range(T)]
        f = (torch.from_numpy(z[f"feats{b}"]).float() / scale).to(feat_dtype).to(device)
        feats.append(f if b == 0 else [f[t][None] for t in range(T)])      # both accepted forms
    return targets, images, feats


def _unpack(a, width):
    return np.unpackbits(a, axis=-1)[..., :width].astype(np.float32)


def check_mined(mined, b):
    """test_mining_vs_reference's rule on the fixture's resized features and stride-4 boxes; -> ambiguous rows."""
    z = gold()
    T = int(z["target_meta"][1])
    err = z["cdist_abs_err"].item()
    feats = torch.from_numpy(z[f"feats_ds{b}"])
    boxes = torch.from_numpy(z[f"box4{b}"])
    p = torch.from_numpy(z[f"pairs{b}"])
    got = mined.to_lists()
    assert len(got) == boxes.shape[0] and all(len(g) == T - 1 for g in got)
    rows = single = 0
    for g in range(boxes.shape[0]):
        for t in range(T - 1):
            sel = p[(p[:, 0] == g) & (p[:, 1] == t)]
            wc, wn = sel[:, 2:4], sel[:, 4:6]
            gc, gn = (v.cpu() for v in got[g][t])
            assert gc.shape == wc.shape and gn.shape == wn.shape, (b, g, t)
            if wc.shape[0] == 0:
                continue
            assert torch.equal(gc.long(), wc.long()), (b, g, t)
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
    return rows - single


def check_targets(out, device=CPU):
    z = gold()
    B, T, D, Hp, Wp, _ = (int(v) for v in z["target_meta"])
    h, w = Hp // 4, Wp // 4
    assert len(out) == B
    ambiguous = 0
    for b, t in enumerate(out):
        G = z[f"labels{b}"].shape[0]
        assert G == int(z[f"valid{b}"].sum())
        for k in ("labels", "ids"):
            assert np.array_equal(t[k].cpu().numpy(), z[f"{k}{b}"]), k
        for k in ("box_masks", "masks"):
            assert t[k].dtype == torch.float32 and tuple(t[k].shape) == (G, T, h, w)
            assert np.array_equal(t[k].cpu().numpy(), _unpack(z[f"{k}{b}"], w)), k
        for k in ("left_bounds", "right_bounds", "top_bounds", "bottom_bounds"):
            assert t[k].dtype == torch.float32 and np.array_equal(t[k].cpu().numpy(), z[f"{k}{b}"]), k
        sim = t["color_similarities"]
        assert tuple(sim.shape) == (G, T, 8, h, w) and sim.stride(0) == 0      # one map shared by the instances
        np.testing.assert_allclose(sim[0].cpu().numpy(), z[f"sim{b}"], rtol=1e-5, atol=1e-6)
        assert len(t["temporal_pairs"]) == G                                   # one entry per returned target
        ambiguous += check_mined(t["temporal_pairs"], b)
    # the reference's debug counters (:503-550), summed over the clips as its forward does (:362-366)
    total = sum(float(t["total_temp_pair"]) for t in out)
    pos = sum(float(t["pos_temp_pair"]) for t in out)
    want = sum(z[f"counters{b}"] for b in range(B))
    assert total == want[0]
    assert abs(pos - want[1]) <= ambiguous
    assert all(t["total_temp_pair"].device.type == device.type for t in out)
    return ambiguous


def padded_images(images, device=CPU):
    z = gold()
    Hp, Wp = (int(v) for v in z["target_meta"][3:5])
    pad = torch.zeros(len(images), 3, Hp, Wp, device=device)
    for i, im in enumerate(images):
        pad[i, :, :im.shape[1], :im.shape[2]] = im.float()
    return pad


# -------------------------------------------------------------------------------------------------------------------
# inference tests
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_inference_vs_reference(name):
    m, out, padded, image, output = infer_case(name)
    res = m(out, padded, image, output)
    check_inference(res, name)
    check_packed(m(out, padded, image, output, packed=True), res, output[1])


def test_inference_default_output_size_and_batch():
    """output_size defaults to the image size (case b); only clip 0 of a batch is used."""
    m, out, padded, image, output = infer_case("b")
    assert output == image
    two = {k: torch.cat([v, torch.zeros_like(v)]) for k, v in out.items()}
    check_inference(m(two, padded, image), "b")


def test_inference_one_query_under_two_classes():
    z = gold()
    q = z["a_queries"]
    assert len(set(q.tolist())) < len(q)


def test_inference_no_queries():
    m = VideoMaskFormerInference(5)
    out = {"pred_logits": torch.zeros(1, 0, 6), "pred_masks": torch.zeros(1, 0, 3, 8, 12)}
    assert m(out, (32, 48), (30, 41), (23, 31)) == {"image_size": (23, 31), "pred_scores": [], "pred_labels": [],
                                                    "pred_masks": []}
    assert m(out, (32, 48), (30, 41), packed=True) == {"image_size": (30, 41), "pred_scores": [], "pred_labels": [],
                                                       "pred_masks": [], "packed": True}


def test_inference_rejects_bad_arguments():
    m, out, padded, image, output = infer_case("a")
    with pytest.raises(ValueError):
        m(out, padded, (padded[0] + 1, image[1]), output)
    with pytest.raises(ValueError):
        VideoMaskFormerInference(4)(out, padded, image, output)


def test_from_config():
    import types
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(SEM_SEG_HEAD=types.SimpleNamespace(NUM_CLASSES=40)))
    m = VideoMaskFormerInference.from_config(cfg)
    assert m.num_classes == 40 and m.test_topk_per_video == 10


@pytest.mark.parametrize("width", [1, 31, 32, 33, 65])
def test_pack_roundtrip(width):
    g = torch.Generator().manual_seed(width)
    m = torch.rand(2, 3, width, generator=g) < 0.5
    m[..., -1] = True
    words = pack_mask_bits(m)
    assert words.dtype == torch.int32 and words.shape[-1] == (width + 31) // 32
    assert torch.equal(unpack_mask_bits(words, width), m)
    x = width - 1
    assert ((words[..., x // 32].long() >> (x % 32)) & 1).all()               # bit x % 32 of word x // 32
    if width % 32:
        assert not (words[..., -1].long() & 0xFFFFFFFF >> (width % 32) << (width % 32)).any()


# -------------------------------------------------------------------------------------------------------------------
# target tests
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_instances", [False, True], ids=["dicts", "instances"])
def test_weaksup_targets_vs_reference(as_instances):
    targets, images, feats = clip_inputs(as_instances=as_instances)
    out = prepare_video_weaksup_targets(targets, images, feats, num_frames=3)
    check_targets(out)


def test_lab_vs_reference():
    _, images, _ = clip_inputs()
    lab = vt._images_lab_torch(padded_images(images), 4)
    torch.testing.assert_close(lab, torch.from_numpy(gold()["lab"]), rtol=1e-6, atol=1e-5)


def test_feat_resize_bitwise():
    z = gold()
    _, _, feats = clip_inputs()
    for b, f in enumerate(feats):
        f = f if torch.is_tensor(f) else torch.cat(f)
        assert np.array_equal(feat_resize_pad(f, (64, 64), (16, 16)).numpy(), z[f"feats_ds{b}"])
    with pytest.raises(ValueError):
        feat_resize_pad(torch.zeros(2, 65, 10), (64, 64), (16, 16))


def test_targets_without_features_and_empty_clip():
    targets, images, _ = clip_inputs()
    out = prepare_video_weaksup_targets(targets, images, None, num_frames=3)
    assert all(t["temporal_pairs"] is None and t["total_temp_pair"] is None and t["pos_temp_pair"] is None for t in out)
    z = gold()
    assert np.array_equal(out[0]["box_masks"].numpy(), _unpack(z["box_masks0"], 16))
    empty = [[{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64),
               "ids": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 44, 60, dtype=torch.bool),
               "image_size": (44, 60)} for _ in range(3)]]
    feats = [torch.zeros(3, 8, 44, 60)]
    t = prepare_video_weaksup_targets(empty, images[:3], feats, num_frames=3)[0]
    assert tuple(t["box_masks"].shape) == (0, 3, 16, 16) and tuple(t["color_similarities"].shape) == (0, 3, 8, 16, 16)
    assert len(t["temporal_pairs"]) == 0 and float(t["total_temp_pair"]) == 0 and float(t["pos_temp_pair"]) == 0
    with pytest.raises(ValueError):
        prepare_video_weaksup_targets(targets, images, None, num_frames=2)


def test_absent_instance_rasters():
    """An absent instance's zero box is the single full-resolution pixel (0, 0): nothing at stride 4, full-width
    bounds; it still counts as a target while another frame holds it (clip 0, the instance with id 3)."""
    targets, images, _ = clip_inputs()
    t = prepare_video_weaksup_targets(targets, images, None, num_frames=3)[0]
    g = int((t["ids"] == -1).any(1).nonzero()[0])
    assert t["ids"][g].tolist() == [3, -1, 3]
    assert not t["box_masks"][g, 1].any() and t["box_masks"][g, 0].any()
    assert (t["left_bounds"][g, 1] == 0).all() and (t["right_bounds"][g, 1] == 16).all()
    assert (t["top_bounds"][g, 1] == 0).all() and (t["bottom_bounds"][g, 1] == 16).all()


def test_targets_feed_the_criterion():
    """VideoWeakTargets takes the prepared dicts as they are: shared similarity, one pair entry per target."""
    from bm2f_amd.video_criterion import VideoWeakTargets
    targets, images, feats = clip_inputs()
    out = prepare_video_weaksup_targets(targets, images, feats, num_frames=3)
    tg = VideoWeakTargets(out, CPU, 0.3)
    assert tg.shared and tg.pairs().P == sum(int(t["total_temp_pair"]) for t in out)


def test_video_targets_vs_reference():
    z = gold()
    targets, _, _ = clip_inputs()
    for inst in (False, True):
        tg = clip_inputs(as_instances=True)[0] if inst else targets
        out = prepare_video_targets(tg, (64, 64), 3)
        for b, t in enumerate(out):
            assert np.array_equal(t["labels"].numpy(), z[f"labels{b}"])
            assert np.array_equal(t["ids"].numpy(), z[f"ids{b}"])
            assert t["masks"].dtype == torch.float32
            assert np.array_equal(t["masks"].numpy(), _unpack(z[f"full_masks{b}"], 64))


# -------------------------------------------------------------------------------------------------------------------
# C ABI: bad arguments are refused before any HIP call (fake pointers never reach a kernel)
# -------------------------------------------------------------------------------------------------------------------
def test_capi_rejects_bad_arguments_without_gpu():
    from bm2f_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    ok = dict(logits=p, dtype=0, slots=p, nsel=None, Q=12, S=10, T=3, h=8, w=12, Hp=32, Wp=48, Hc=30, Wc=41, Ho=23,
              Wo=31, packed=0, out=p, stream=None)

    def video(**kw):
        a = dict(ok, **kw)
        rc = lib.m2f_infer_video(*a.values())
        return rc, lib.m2f_last_error()

    assert video(logits=None) == (1, b"m2f_infer_video: null pointer")
    assert video(out=None)[0] == 1 and video(slots=None)[0] == 1
    rc, msg = video(dtype=7)
    assert rc == 3 and b"dtype" in msg
    assert video(T=0)[0] == 1 and video(Ho=-1)[0] == 1
    rc, msg = video(Hc=33)
    assert rc == 1 and b"exceeds the padded size" in msg
    assert video(packed=2)[0] == 1
    rc, msg = video(out=ctypes.c_void_p((1 << 20) + 2))
    assert rc == 1 and b"aligned" in msg
    assert video(T=65536)[0] == 3 and video(S=65536)[0] == 3
    assert video(h=1 << 16, w=1 << 16)[0] == 3

    def resize(*a):
        rc = lib.m2f_feat_resize_pad(*a)
        return rc, lib.m2f_last_error()

    assert resize(None, 0, 24, 44, 60, 64, 64, 16, 16, p, None)[0] == 1
    assert resize(p, 0, 24, 44, 60, 64, 64, 16, 16, None, None)[0] == 1
    rc, msg = resize(p, 5, 24, 44, 60, 64, 64, 16, 16, p, None)
    assert rc == 3 and b"dtype" in msg
    rc, msg = resize(p, 0, 24, 65, 60, 64, 64, 16, 16, p, None)
    assert rc == 1 and b"exceeds the padded size" in msg
    assert resize(p, 0, 0, 44, 60, 64, 64, 16, 16, p, None)[0] == 1
    assert resize(p, 0, 24, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 16, 16, p, None)[0] == 3


def test_option_infer_video_cap():
    from bm2f_amd import _native
    assert _native.get_option("infer_video_cap") == -1
    with _native.options(infer_video_cap=0):
        assert _native.get_option("infer_video_cap") == 0
    assert _native.get_option("infer_video_cap") == -1
