"""The inputs of tests/test_attn_range_gpu.py do what they claim, and a correct 16-bit kernel passes on them (no GPU).

1. Block-max steps: in fp64, the per-row maxima of s * scale * log2(e) over the open keys of each 64-key block step
   as the profile says, so the forward kernel's lazy rescale (decoder.hip kLazyLog2 = 8) takes the branch the GPU
   case is named for; with the ``torch.randn`` inputs of the older tests no step after a row's first open block ever
   exceeds 8 (the gap these cases close).
2. Floor: an fp64 emulation of the roundings any flash-style 16-bit kernel makes stays within one third of the GPU
   test's bars, so a failure there is the kernel's and not the inputs'.
"""
import pytest
import torch

import attn_range_cases as arc
from oracle.decoder_ref import ref_masked_attention

LQ, LK, H = 48, 640, 8
SEEDS = arc.SEEDS


def _steps(profile, dtype=torch.float32, seed=None):
    """-> (block maxima (H, Lq, nblocks), rows with c = +1, rows with c = -1), special mask rows left out."""
    q, k, v, blocked, _ = arc.make_case(profile, dtype, LQ, LK, H, SEEDS[profile] if seed is None else seed)
    bm = arc.block_maxima(arc.log2_scores(q, k, blocked, H))
    c = arc.row_coeff(LQ)
    plain = torch.ones(LQ, dtype=torch.bool)
    plain[[arc.ROW_LAST_ONLY, arc.ROW_FIRST_ONLY, arc.ROW_OPEN]] = False
    return bm, (c == 1.0) & plain, (c == -1.0) & plain


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_up_every_block_rescales_rising_rows_only(dt):
    bm, pos, neg = _steps("up", arc.DTYPES[dt])
    assert torch.isfinite(bm[:, pos | neg]).all()          # every block has an open key
    rise = bm[..., 1:] - bm[..., :-1]
    assert pos.sum() >= 16 and neg.sum() >= 16
    assert rise[:, pos].min().item() > arc.LAZY_LOG2, rise[:, pos].min().item()
    # the odd rows of the same 16-row tiles fall: nothing after their first block moves their max
    assert rise[:, neg].max().item() < 0.0, rise[:, neg].max().item()
    for tile in range(LQ // 16):                           # both kinds in every MFMA tile: the wave-uniform __any
        rows = torch.arange(16 * tile, 16 * tile + 16)
        assert pos[rows].any() and neg[rows].any()


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_down_rises_for_the_negated_rows(dt):
    bm, pos, neg = _steps("down", arc.DTYPES[dt])
    rise = bm[..., 1:] - bm[..., :-1]
    assert rise[:, neg].min().item() > arc.LAZY_LOG2
    assert rise[:, pos].max().item() < 0.0


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_slow_uses_the_stale_max_then_rescales(dt):
    bm, pos, _ = _steps("slow", arc.DTYPES[dt])
    b = bm[:, pos]
    rise = b[..., 1:] - b[..., :-1]
    small = (rise > 0.0) & (rise < arc.LAZY_LOG2)
    assert small.any(-1).all()                             # every such row: a block taken against the stale max
    assert (b[..., -1] - b[..., 0]).min().item() > arc.LAZY_LOG2   # ... and a rescale later
    # walk the kernel's rule: at least one block on the stale max (0 < rise over the running max <= 8) and one
    # rescale of a nonzero accumulator per row
    for row in b.reshape(-1, b.shape[-1]):
        m_run, stale, rescale = row[0].item(), 0, 0
        for m_blk in row[1:].tolist():
            if m_blk > m_run + arc.LAZY_LOG2:
                m_run, rescale = m_blk, rescale + 1
            elif m_blk > m_run:
                stale += 1
        assert stale >= 1 and rescale >= 1


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_spike_chunk_towers_over_the_others(dt):
    q, k, v, blocked, _ = arc.make_case("spike", arc.DTYPES[dt], LQ, LK, H, SEEDS["spike"])
    chunk = 128                                            # the forward's default chunk at these sizes
    cm = arc.block_maxima(arc.log2_scores(q, k, blocked, H), chunk)
    s0 = arc.spike_start(LK)
    assert s0 // chunk == (s0 + arc.SPIKE_KEYS - 1) // chunk
    sc = s0 // chunk
    c = arc.row_coeff(LQ)
    rows = (c == 1.0) & ~blocked[0][:, s0:s0 + arc.SPIKE_KEYS].all(-1)   # rising rows that see a spike key
    assert rows.sum() >= 12
    others = cm.clone()
    others[..., sc] = float("-inf")
    excess = (cm[..., sc] - others.amax(-1))[:, rows]
    assert excess.min().item() > 40.0, excess.min().item()


@pytest.mark.parametrize("B,Lq,Lk", [(2, 100, 1024), (1, 37, 4096 + 17), (3, 200, 300)])
def test_randn_inputs_never_step_past_the_lazy_threshold(B, Lq, Lk):
    """The inputs of test_decoder_gpu.test_masked_attention: after a row's first open block no block max exceeds
    the running max by 2^8, so the only rescale those tests ever run multiplies zeros by alpha = 0."""
    from test_decoder_gpu import _attn_case
    q, k, v, blocked = _attn_case(torch.device("cpu"), B, Lq, Lk, H, torch.float32, 0.6, Lq + Lk)
    worst = float("-inf")
    for b in range(B):
        bm = arc.block_maxima(arc.log2_scores(q[b:b + 1], k[b:b + 1], blocked[b:b + 1], H))
        run = torch.cummax(bm, -1).values                 # the running max is at most this (lazy: it may lag)
        step = bm[..., 1:] - run[..., :-1]
        step = step[torch.isfinite(run[..., :-1]) & torch.isfinite(bm[..., 1:])]
        worst = max(worst, step.max().item())
    assert worst < arc.LAZY_LOG2, worst


# ------------------------------------------------------------------------------------------------------
# the floor of an ideal 16-bit flash-style kernel
# ------------------------------------------------------------------------------------------------------
OUT_BAR = {"bf16": 2e-2, "f16": 4e-3}                      # the GPU test's bars (gradients: 3x)


def _reference(q, k, v, blocked, gout):
    qd, kd, vd = (t.double().clone().requires_grad_() for t in (q, k, v))
    ref = ref_masked_attention(qd, kd, vd, blocked, H)
    ref.backward(gout.double())
    return ref.detach(), qd.grad, kd.grad, vd.grad


def _ideal_16bit(q, k, v, blocked, gout, dtype):
    """fp64 arithmetic with the roundings a flash-style kernel in ``dtype`` cannot avoid: out; delta from the
    rounded out; P as the MFMA operand of dV; dS as the MFMA operand of dQ / dK; the three gradients."""
    def rnd(t):
        return t.to(dtype).double()

    Lq, Lk = q.shape[1], k.shape[1]
    qh, kh, vh, gh = (t[0].double().view(-1, H, arc.HEAD_DIM).transpose(0, 1) for t in (q, k, v, gout))
    s = (qh @ kh.transpose(1, 2) * arc.SCALE).masked_fill(blocked[0][None], float("-inf"))
    p = s.softmax(-1)
    out = rnd(p @ vh)
    delta = (gh * out).sum(-1, keepdim=True)
    dv = rnd(rnd(p).transpose(1, 2) @ gh)
    ds = rnd(p * (gh @ vh.transpose(1, 2) - delta))
    dq = rnd(ds @ kh * arc.SCALE)
    dk = rnd(ds.transpose(1, 2) @ qh * arc.SCALE)

    def merge(t):
        return t.transpose(0, 1).reshape(1, -1, H * arc.HEAD_DIM)

    return merge(out), merge(dq), merge(dk), merge(dv)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("profile", arc.PROFILES)
def test_ideal_16bit_kernel_is_within_a_third_of_the_bars(profile, dt):
    dtype = arc.DTYPES[dt]
    case = arc.make_case(profile, dtype, LQ, LK, H, SEEDS[profile])
    want = _reference(*case)
    got = _ideal_16bit(*case, dtype)
    errs = {n: arc.max_rel(g, w) for n, g, w in zip(("out", "dq", "dk", "dv"), got, want)}
    print(f"{profile} {dt} ideal-kernel floor: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs["out"] <= OUT_BAR[dt] / 3, errs
    for n in ("dq", "dk", "dv"):
        assert errs[n] <= (3 * OUT_BAR[dt]) / 3, errs


def test_special_rows_and_rounding():
    q, k, v, blocked, gout = arc.make_case("up", torch.bfloat16, LQ, 200, H, 3)
    assert q.dtype == k.dtype == v.dtype == gout.dtype == torch.bfloat16
    b = blocked[0]
    assert not b[:, 0][torch.arange(LQ) != arc.ROW_LAST_ONLY].any()
    assert b[arc.ROW_LAST_ONLY].sum() == 199 and not b[arc.ROW_LAST_ONLY, -1]
    assert b[arc.ROW_FIRST_ONLY].sum() == 199 and not b[arc.ROW_FIRST_ONLY, 0]
    assert not b[arc.ROW_OPEN].any()
    c = arc.row_coeff(LQ)
    assert {c[arc.ROW_LAST_ONLY].item(), c[arc.ROW_FIRST_ONLY].item(), c[arc.ROW_OPEN].item()} == {1.0, -1.0}
    assert not b.all(-1).any()                              # no fully blocked row
    # the magnitude sits in q: keys stay small
    assert q.float().abs().max() > 10 * k.float().abs().max()


# ------------------------------------------------------------------------------------------------------
# the cases tell a wrong rescale from a right one
# ------------------------------------------------------------------------------------------------------
def _lazy_forward(q, k, v, blocked, rescale_sum=True, rescale_out=True):
    """The forward kernel's blockwise rule in fp64: the running max moves only past 2^8, O and the row sum are
    multiplied by alpha when it does (either multiply can be left out, as a defective kernel would)."""
    s = arc.log2_scores(q, k, blocked, H)                  # (H, Lq, Lk)
    vh = v[0].double().view(-1, H, arc.HEAD_DIM).transpose(0, 1)
    m = s.new_full(s.shape[:2], float("-inf"))
    l = s.new_zeros(s.shape[:2])
    o = s.new_zeros(*s.shape[:2], arc.HEAD_DIM)
    for k0 in range(0, s.shape[-1], arc.BLOCK):
        sb = s[..., k0:k0 + arc.BLOCK]
        m_blk = sb.amax(-1)
        move = m_blk > m + arc.LAZY_LOG2
        m_new = torch.where(move, torch.maximum(m, m_blk), m)
        alpha = torch.exp2(m - torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new)))
        alpha = torch.where(move, alpha, torch.ones_like(alpha))
        m = m_new
        if rescale_out:
            o = o * alpha[..., None]
        if rescale_sum:
            l = l * alpha
        p = torch.exp2(sb - torch.where(torch.isfinite(m), m, torch.zeros_like(m))[..., None])
        l = l + p.sum(-1)
        o = o + p @ vh[:, k0:k0 + arc.BLOCK]
    out = o / l[..., None]
    return out.transpose(0, 1).reshape(1, -1, H * arc.HEAD_DIM)


@pytest.mark.parametrize("profile", arc.PROFILES)
def test_cases_catch_a_rescale_that_skips_the_sum_or_the_output(profile):
    q, k, v, blocked, gout = arc.make_case(profile, torch.float32, LQ, LK, H, SEEDS[profile])
    want = ref_masked_attention(q.double(), k.double(), v.double(), blocked, H)
    assert arc.max_rel(_lazy_forward(q, k, v, blocked), want) < 1e-9
    loosest_bar = 2e-2                                      # bf16's
    assert arc.max_rel(_lazy_forward(q, k, v, blocked, rescale_sum=False), want) > 5 * loosest_bar
    assert arc.max_rel(_lazy_forward(q, k, v, blocked, rescale_out=False), want) > 5 * loosest_bar
