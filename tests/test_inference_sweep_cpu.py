"""The conditions that make test_inference_sweep_gpu.py meaningful, asserted without a GPU: every synthetic case of
inference_cases.py reaches the branch of csrc/inference.hip it is there for (reach), its expectation is not trivial
(strength) and stays clear of the fp64 ambiguity caps.  A case that stops reaching its branch fails here."""
import numpy as np
import pytest
import torch

import inference_cases as ic
import inference_util as iu
from gen_inference_golden import AMB_CAP, merge_loop


def _n_keep(c, b):
    from bm2f_amd.inference import _keep_lists
    return int(_keep_lists(c.cls[b], c.K, c.thresholds[0])[3])


# ---------------------------------------------------------------------------------------------------------------------
# reach
# ---------------------------------------------------------------------------------------------------------------------
def test_tap_replica_matches_torch():
    """The numpy replica of bilinear_tap picks the source index torch's upsample_bilinear2d reads: interpolating a
    ramp of indices returns values between the replica's i0 and i1."""
    import torch.nn.functional as F
    for n_in, n_out in ((6, 24), (72, 35), (21, 65), (1, 16), (2, 16), (17, 68)):
        ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        got = F.interpolate(ramp, size=(1, n_out), mode="bilinear", align_corners=False).flatten().numpy()
        for d in range(n_out):
            i0, i1 = ic.bilinear_tap(d, np.float32(n_in) / np.float32(n_out), n_in)
            assert i0 <= got[d] <= i1 and i1 - i0 == (i0 < n_in - 1), (n_in, n_out, d)


@pytest.mark.parametrize("name", ic.DIRECT)
def test_direct_cases_read_global_memory(name):
    """use_win == false: at least one 4 x 32 tile's source window exceeds kWinCap = 176 texels."""
    c = ic.get(name)
    assert all((ic.tile_windows(c, b) > ic.WIN_CAP).any() for b in range(c.B))


@pytest.mark.parametrize("name", ic.MIXED)
def test_mixed_batches_take_both_paths(name):
    c = ic.get(name)
    over = [(ic.tile_windows(c, b) > ic.WIN_CAP) for b in range(c.B)]
    assert over[0].any() and not over[1].any()
    # one image is smaller than the batch's output buffer (Ho < out_h): the early return and the row/column guards
    assert c.output_sizes[0][0] < max(s[0] for s in c.output_sizes)


@pytest.mark.parametrize("name", [n for n in ic.NAMES if n not in ic.DIRECT + ic.MIXED])
def test_window_cases_stay_in_lds(name):
    c = ic.get(name)
    assert all((ic.tile_windows(c, b) <= ic.WIN_CAP).all() for b in range(c.B))


def test_many_tiles_case_loops_in_the_combine_kernel():
    """instance_combine_kernel: lane t adds tiles t, t + 64, ...; more than 64 tiles makes the loop run twice."""
    assert ic.instance_tiles(ic.get("many_tiles")) == 67 > 64
    assert ic.instance_tiles(ic.get("out32x32")) == 1 and ic.instance_tiles(ic.get("out25x41")) == 2


def test_class_sweep_covers_every_instantiation():
    """semantic_kernel<KT>, KT = ceil(K / 32) = 1..8, with K = 32 n and 32 n + 1 (the k < K padding) among them."""
    assert {-(-k // 32) for k in ic.K_SWEEP} == set(range(1, 9))
    assert {32, 33, 64, 65, 224, 225, 256} <= set(ic.K_SWEEP)
    assert all(ic.get(f"K{k}").K == k for k in ic.K_SWEEP)


def test_query_sweep_covers_the_chunk_edges():
    """kQC = 32: one partial chunk, exact chunks, one over; kMaxQ = 256 with every query kept (nk == Q)."""
    assert {1, 31, 32, 33, 200, 256} <= set(ic.Q_SWEEP)
    assert _n_keep(ic.get("Q256"), 0) == ic.get("Q256").Q == 256
    assert _n_keep(ic.get("none_kept"), 0) == 0
    assert all(0 < _n_keep(ic.get(f"Q{q}"), 0) < q for q in ic.Q_SWEEP if 1 < q < 256)


def test_selection_edges():
    c = ic.get("w33")
    assert c.topk == c.Q * c.K
    c = ic.get("twins")
    e = ic.expected("twins")[0]
    a, b = ic.twin_queries(c)
    assert a < b and torch.equal(c.cls[0, a], c.cls[0, b]) and torch.equal(c.masks[0, a], c.masks[0, b])
    klass = int(c.cls[0, a].argmax())
    assert klass < c.things
    ka, kb = (e.keep_queries.tolist().index(q) for q in (a, b))
    # the first twin owns a segment, the second wins no pixel
    assert e.counters[ka, 0] > 0 and e.counters[kb, 0] == 0 and e.counters[ka, 1] == e.counters[kb, 1] > 0
    assert [s["category_id"] for s in e.segments_info if s["isthing"]].count(klass) == 1
    assert a not in e.inst_queries and b not in e.inst_queries


# ---------------------------------------------------------------------------------------------------------------------
# strength and caps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", [("fp32", n) for n in ic.NAMES] +
                         [(d, n) for d in ("fp16", "bf16") for n in ic.SIXTEEN_BIT])
def test_expectation_is_strong_and_unambiguous(name, dt):
    c = ic.get(name)
    exp = ic.expected(name, dt)      # runs _assert_separable
    for b, e in enumerate(exp):
        npix = c.output_sizes[b][0] * c.output_sizes[b][1]
        assert e.sem_amb.sum() <= AMB_CAP * npix and (e.pan_amb.sum() <= AMB_CAP * npix or c.twins), (name, b)
        assert e.thr_amb.reshape(c.Q, -1).sum(1).max() <= AMB_CAP * npix, (name, b)
        if name == "none_kept":
            assert e.segments_info == [] and not e.panoptic_seg.any()
        else:
            assert len(e.segments_info) >= 1 and e.panoptic_seg.any(), (name, b)
        if name == "no_things":
            assert e.inst_masks.shape == (0, *c.output_sizes[b])
        else:
            part = e.inst_masks.reshape(len(e.inst_masks), -1).mean(1)
            assert ((part > 0) & (part < 1)).any(), (name, b)
        if c.twins:
            # the exact tie is the only ambiguity the margins flag beyond the cap
            a, _ = ic.twin_queries(c)
            seg = [s["id"] for s in e.segments_info if s["category_id"] == int(c.cls[b, a].argmax())][0]
            assert (e.pan_amb & (e.panoptic_seg != seg) & (e.pan_top != seg)).sum() <= AMB_CAP * npix


def test_panoptic_events_are_reached():
    """Somewhere in the sweep two stuff queries merge into one segment and the overlap threshold drops a query."""
    seen = {"merge": 0, "overlap_drop": 0}
    for name in ic.NAMES:
        c = ic.get(name)
        labels = torch.softmax(c.cls, -1).argmax(-1)
        for b, e in enumerate(ic.expected(name)):
            ev = merge_loop(labels[b, e.keep_queries].tolist(), e.counters.tolist(), c.things)[2]
            seen = {k: v + ev[k] for k, v in seen.items()}
    assert seen["merge"] >= 1 and seen["overlap_drop"] >= 1, seen


@pytest.mark.parametrize("k", ic.K_SWEEP)
def test_ramp_planes_are_pairwise_distinct(k):
    """Score mode on ``cls_ramp``: every two class planes differ somewhere by more than twice the bar, so a permuted
    class index in the epilogue (k = 32 i + (e & 3) + 8 (e >> 2) + 4 lh) cannot pass."""
    c = ic.get(f"K{k}")
    sem = ic.ramp_expected(c)[0].double().flatten(1)
    bar = iu.RTOL * sem.abs().max()
    gap = torch.stack([(sem - sem[i]).abs().amax(1) for i in range(k)])
    gap.fill_diagonal_(float("inf"))
    assert gap.min() > 2 * bar, (k, float(gap.min()), float(bar))


# ---------------------------------------------------------------------------------------------------------------------
# non-finite logits
# ---------------------------------------------------------------------------------------------------------------------
def test_infinite_case_has_no_nan():
    c = ic.get("inf")
    full = ic.full64(c, 0)
    assert c.masks.isinf().sum() == 3 and (full == ic.INF).any() and (full == -ic.INF).any() and not full.isnan().any()
    # an infinite texel reaches kept and instance queries alike
    e = ic.expected("inf")[0]
    hit = full.isinf().flatten(1).any(1).nonzero().flatten().tolist()
    assert set(hit) & set(e.keep_queries.tolist()) and len(hit) == 3


def test_nan_case_on_the_cpu_path():
    """What the GPU test relies on: torch.argmax gives an all-NaN pixel to the first kept query, the segment list is
    the clean case's (so its candidates apply), and the NaN pixels outnumber the ambiguous ones."""
    from bm2f_amd.inference import _keep_lists, _panoptic_pixels_cpu, full_resolution_logits
    c, masks, reach, cpu, counters = ic.nan_case()
    e = ic.expected("nan_clean")[0]
    order, kscore, _, n_keep = _keep_lists(c.cls[0], c.K, c.thresholds[0])
    full = full_resolution_logits(masks[0], c.padded, c.image_sizes[0], c.output_sizes[0])
    winner, inside, _ = _panoptic_pixels_cpu(full, order, kscore, int(n_keep))
    assert int(n_keep) > 1 and not winner.numpy()[reach].any() and not inside.numpy()[reach].any()
    assert cpu["panoptic_seg"][1] == e.segments_info and not cpu["panoptic_seg"][0].numpy()[reach].any()
    assert counters[0, 0] >= reach.sum() > int(e.pan_amb.sum()) + int(e.thr_amb[e.keep_queries].sum())
    assert cpu["sem_seg"].isnan().numpy()[:, reach].all() and not cpu["sem_seg"].isnan().numpy()[:, ~reach].any()
