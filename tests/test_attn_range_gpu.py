"""Masked attention (bm2f_amd/csrc/decoder.hip) where the softmax max moves between key blocks: the score ranges of
a trained decoder's peaked cross-attention (tens to over a hundred log2 units per row) instead of the unit-variance
scores of ``torch.randn`` inputs, and the query counts the other tests leave out.

Inputs: tests/attn_range_cases.py (tests/test_attn_range_cpu.py proves what they exercise, and that an ideal 16-bit
kernel stays within a third of the bars here).  Reference: oracle.decoder_ref.ref_masked_attention on the fp64 copy of
the dtype-rounded inputs, gradients by autograd.  Metric: max|a - b| / max|b|.  Bars: the project's own for 16-bit
(bf16 2e-2, f16 4e-3; gradients 3x); for fp32 max(2e-5, 2 err) per tensor (gradients: 6e-5 in place of 2e-5), ``err``
being the error of the same restatement run in fp32 on the same device: at scores near 100 the fp32 ulp is 7.6e-6
in the exponent, so torch's own fp32 softmax is 3-8e-6 off and a fixed 2e-5 leaves too little room.
"""
import functools

import pytest
import torch

import attn_range_cases as arc
from oracle.decoder_ref import pack_bits, ref_masked_attention

pytestmark = pytest.mark.gpu

H = 8
OUT_BAR = {"bf16": 2e-2, "f16": 4e-3}
NAMES = ("out", "dq", "dk", "dv")
# two roundings of the output format (f16: the 2e-3 of test_masked_attention_combine_sparse_chunks); fp32: the
# project's fp32 tolerance, the two forms adding up to 33 fp32 partials in different orders
AGREE = {"f16": 2e-3, "bf16": 2 ** -6, "f32": 2e-5}


@functools.lru_cache(maxsize=None)
def _case(profile, dt, Lq, Lk, seed):
    """CPU inputs and their fp64 reference (out, dq, dk, dv), computed once per case and never modified."""
    q, k, v, blocked, gout = arc.make_case(profile, arc.DTYPES[dt], Lq, Lk, H, seed)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ref = ref_masked_attention(qd, kd, vd, blocked, H)
    ref.backward(gout.double())
    return (q, k, v, blocked, gout), (ref.detach(), qd.grad, kd.grad, vd.grad)


@functools.lru_cache(maxsize=None)
def _fp32_restatement_error(device, profile, Lq, Lk, seed):
    """max-rel error per tensor of ref_masked_attention run in fp32 on the device, against fp64."""
    (q, k, v, blocked, gout), want = _case(profile, "f32", Lq, Lk, seed)
    qf, kf, vf = (t.to(device).requires_grad_() for t in (q, k, v))
    ref = ref_masked_attention(qf, kf, vf, blocked.to(device), H)
    ref.backward(gout.to(device))
    got = (ref.detach(), qf.grad, kf.grad, vf.grad)
    return tuple(arc.max_rel(g.cpu(), w) for g, w in zip(got, want))


def _seed(Lq, Lk, profile):
    return arc.SEEDS[profile] if (Lq, Lk) == (48, 640) else 5


def _run(device, inputs, backward=True, **opts):
    """The kernels on ``inputs`` under native options ``opts`` -> (out, dq, dk, dv) on the device."""
    from bm2f_amd import _native, decoder_ops
    q, k, v, blocked, gout = inputs
    bits = pack_bits(blocked).to(device)
    qa, ka, va = (t.to(device).requires_grad_() for t in (q, k, v))
    with _native.options(**opts):
        out = decoder_ops.masked_attention(qa, ka, va, bits, H)
        if not backward:
            return (out.detach(),)
        out.backward(gout.to(device))
    return out.detach(), qa.grad, ka.grad, va.grad


def _check(device, label, key, got):
    """Finite, within the bars, and the one-open-key rows equal to that key's value row."""
    profile, dt, Lq, Lk, seed = key
    (q, k, v, blocked, gout), want = _case(*key)
    restate = _fp32_restatement_error(device, profile, Lq, Lk, seed) if dt == "f32" else None
    failures = []
    for i, (name, g, w) in enumerate(zip(NAMES, got, want)):
        assert torch.isfinite(g).all(), f"{label}: {name} has non-finite values"
        err = arc.max_rel(g.cpu(), w)
        if dt == "f32":
            bar = max(2e-5 if i == 0 else 6e-5, 2 * restate[i])
            print(f"{label} {name}: err {err:.3e} bar {bar:.3e} (fp32 restatement {restate[i]:.3e})")
        else:
            bar = OUT_BAR[dt] * (1 if i == 0 else 3)
            print(f"{label} {name}: err {err:.3e} bar {bar:.3e}")
        if not err < bar:
            failures.append((name, err, bar))
    assert not failures, f"{label}: {failures}"
    out = got[0].cpu()
    eps = torch.finfo(arc.DTYPES[dt]).eps
    for row, key_row in ((arc.ROW_FIRST_ONLY, 0), (arc.ROW_LAST_ONLY, Lk - 1)):
        if row < Lq:
            torch.testing.assert_close(out[0, row].double(), v[0, key_row].double(), rtol=4 * eps, atol=1e-30,
                                       msg=lambda m: f"{label}: row {row} sees only key {key_row}: {m}")


def _plan(Lq, Lk):
    from bm2f_amd import decoder_ops
    return decoder_ops._plan(1, Lq, Lk, H)


# ------------------------------------------------------------------------------------------------------
# 1. every block transition inside one workgroup
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("profile", arc.PROFILES)
def test_rescale_in_one_chunk(device, profile, dt):
    from bm2f_amd import _native
    Lq, Lk = 48, 640
    key = (profile, dt, Lq, Lk, _seed(Lq, Lk, profile))
    opts = dict(mattn_fwd_minblk=16, mattn_bwd_minblk=16)
    with _native.options(**opts):
        assert _plan(Lq, Lk)[1] == 1          # ten 64-key blocks, nine transitions, one workgroup per head
    _check(device, f"one-chunk {profile} {dt}", key, _run(device, _case(*key)[0], **opts))


# ------------------------------------------------------------------------------------------------------
# 2. chunked, both combine kernels
# ------------------------------------------------------------------------------------------------------
def _both_combines(device, key, min_chunks):
    profile, dt, Lq, Lk, _ = key
    assert _plan(Lq, Lk)[1] >= min_chunks, _plan(Lq, Lk)
    outs = []
    for combine in (0, 1):
        got = _run(device, _case(*key)[0], mattn_combine=combine)
        _check(device, f"chunked Lk={Lk} combine={combine} {profile} {dt}", key, got)
        outs.append(got[0].float())
    torch.testing.assert_close(outs[1], outs[0], rtol=AGREE[dt], atol=AGREE[dt])


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("profile", arc.PROFILES)
def test_chunked_both_combines(device, profile, dt):
    Lq, Lk = 48, 640
    _both_combines(device, (profile, dt, Lq, Lk, _seed(Lq, Lk, profile)), 2)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("profile", ["spike", "up"])
def test_many_chunks_ragged_tail(device, profile, dt):
    # 17 chunks of 128 keys, the last with 5.  ``up`` reaches a[j] = 384 here, so the keys grow to ~7 and dq = dS @ k
    # starts to cancel: the ideal 16-bit kernel of test_attn_range_cpu is at 2.5e-2 (bf16) on dq, the kernel at 4.2e-2
    # of the 6e-2 bar -- the largest error / bar ratio of this file
    Lq, Lk = 48, 2053
    _both_combines(device, (profile, dt, Lq, Lk, _seed(Lq, Lk, profile)), 16)


# ------------------------------------------------------------------------------------------------------
# 3. backward variants at range
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [16, 32])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("profile", ["up", "spike"])
def test_backward_key_tiles_at_range(device, profile, dt, keys):
    Lq, Lk = 48, 640
    key = (profile, dt, Lq, Lk, _seed(Lq, Lk, profile))
    _check(device, f"bwd_keys={keys} {profile} {dt}", key, _run(device, _case(*key)[0], mattn_bwd_keys=keys))


@pytest.mark.parametrize("dq", [0, 1, 2])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_dq_modes_at_range(device, dt, dq):
    Lq, Lk = 200, 640
    key = ("up", dt, Lq, Lk, _seed(Lq, Lk, "up"))
    _check(device, f"dq_atomic={dq} Lq={Lq} {dt}", key, _run(device, _case(*key)[0], mattn_dq_atomic=dq))


# ------------------------------------------------------------------------------------------------------
# 4. query-count edges: every forward instantiation (1, 2, 4, 8 tiles per wave) and backward dQ path at its limits
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Lq", [(dt, Lq) for dt in ("bf16", "f32")
                                   for Lq in (1, 16, 17, 64, 65, 208, 209, 256, 257, 336)] + [("bf16", 512)])
def test_query_count_edges(device, dt, Lq):
    Lk = 200                                   # three blocks and an 8-key tail
    key = ("up", dt, Lq, Lk, _seed(Lq, Lk, "up"))
    _check(device, f"Lq={Lq} {dt}", key, _run(device, _case(*key)[0]))


# ------------------------------------------------------------------------------------------------------
# 5. limits
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_513_queries_are_rejected(device, dt):
    from bm2f_amd import _native
    inputs = arc.make_case("up", arc.DTYPES[dt], 513, 200, H, 5)
    with pytest.raises(_native.NativeError, match="513 queries"):
        _run(device, inputs, backward=False)


def test_fp32_backward_stops_at_336_queries(device):
    """bwd_lds_bytes: the fp32 backward (LDS-atomic dQ above 208 queries) holds 412 B of LDS per padded query row
    + 21,248 B: 159,680 B at Lqp = 336, 166,272 B at 352, over the 160 KB of a workgroup.  The forward has no such
    limit: fp32 at 352 queries runs forward to the bar and fails with M2F_EUNSUPPORTED only in backward."""
    from bm2f_amd import _native, decoder_ops
    Lq, Lk = 352, 200
    key = ("up", "f32", Lq, Lk, 5)
    (q, k, v, blocked, gout), want = _case(*key)
    qa, ka, va = (t.to(device).requires_grad_() for t in (q, k, v))
    out = decoder_ops.masked_attention(qa, ka, va, pack_bits(blocked).to(device), H)
    assert torch.isfinite(out).all()
    err = arc.max_rel(out.detach().cpu(), want[0])
    bar = max(2e-5, 2 * _fp32_restatement_error(device, "up", Lq, Lk, 5)[0])
    print(f"Lq={Lq} f32 forward out: err {err:.3e} bar {bar:.3e}")
    assert err < bar
    with pytest.raises(_native.NativeError, match="LDS"):
        out.backward(gout.to(device))


# ------------------------------------------------------------------------------------------------------
# 6. the XCD mapping only renames workgroups
# ------------------------------------------------------------------------------------------------------
def test_xcd_mapping_bitwise_at_range(device):
    Lq, Lk = 48, 2000                          # forward: 16 chunks of 128 keys; backward: 8 of 256
    chunk_len, nch, _, _ = _plan(Lq, Lk)
    assert (1 * nch) % 8 == 0, (chunk_len, nch)   # else the host keeps the plain mapping whatever the option says
    inputs = _case("up", "f16", Lq, Lk, 5)[0]
    plain, mapped = (_run(device, inputs, mattn_xcd=x) for x in (0, 1))
    for name, a, b in zip(NAMES, plain, mapped):
        assert torch.equal(a, b), name
