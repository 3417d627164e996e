"""Shifted-window attention (csrc/window_attn.hip) on the GPU at every window size it is built for: all eight tile
counts NT = ceil(ws^2 / 16) in fp32, fp16 and bf16, forward and backward, against tests/swin_ref.py in fp64 on the values
the device tensors hold.  Cases and inputs: tests/window_attn_cases.py; tests/test_window_attn_sweep_cpu.py shows that
an indexing mistake in the bias gather, the shift or the scale moves these outputs by 0.05 of their max or more.

Bounds, on rel_dist = max |got - want| / max |want| per tensor (out, dqkv, dtable):

16-bit I/O: the standing rule tol(floor) = max(1e-3, 2 floor), the floor being window_attention_torch's distance from
fp64 on the same device in the same I/O precision.

fp32 I/O: max(K32 * floor, A32), never above 1e-4, with the floor of the torch fp32 path for the same case and tensor.
The kernel may be worse than torch by __expf's argument scaling, whose error grows with |s - m|, and by the MFMA's
summation order.  K32 and A32 come from one run of this module on an MI355X (shifted-window attention,
"Sweep over the window sizes").  Over the 47 cases and three tensors of that run, in fp32:

    kernel distance   9.0e-8 .. 7.2e-7, and 1.3e-6 .. 5.2e-6 in the wide-score cases
    torch floor       5.9e-8 .. 1.0e-6, and 5.0e-7 .. 2.8e-6 in the wide-score cases
    distance / floor  at most 4.0 (wide ws 3, dtable: 1.99e-6 against 4.98e-7; its dqkv: 5.22e-6 against 1.43e-6)

K32 = 8 is twice that worst ratio.  A32 = 2e-6 is 2.8 times the largest distance outside the wide-score cases (7.2e-7)
and keeps a tensor whose torch floor happens to be small (5.9e-8 at ws 3) on the scale of fp32 rounding.  The largest
bound in force is 8 x 2.8e-6 = 2.2e-5.  All 48 instantiations agreed with fp64 within these bounds in that run.
"""
import pytest
import torch

from swin_ref import rel_dist
from test_swin_cpu import tol
from window_attn_cases import CASES, DTYPES, TAIL_CASES, case_id, dtypes_of, make_inputs, reference, tail_inputs

pytestmark = pytest.mark.gpu

K32, A32, CAP32 = 8.0, 2e-6, 1e-4
NAMES = ("out", "dqkv", "dtable")
BY_ID = {case_id(c): c for c in CASES}
SWEEP6, SWEEP10, SWEEP3 = (BY_ID[f"sweep-ws{ws}-nt{nt}-shift{ws // 2}-b2h2-2x3"] for ws, nt in ((6, 3), (10, 7), (3, 1)))


def fp32_bound(floor):
    return min(max(K32 * float(floor), A32), CAP32)


def bound_of(name, floor):
    return fp32_bound(floor) if name == "fp32" else tol(floor)


def run(case, qkv, table, gout, device, torch_path=False):
    from bm2f_amd import window_attention
    from bm2f_amd.swin import window_attention_torch
    q = qkv.to(device).requires_grad_()
    t = table.to(device).requires_grad_()
    fn = window_attention_torch if torch_path else window_attention
    out = fn(q, t, case.nH, case.ws, case.shift, case.scale)
    out.backward(gout.to(device))
    return out.detach(), q.grad, t.grad


def check_against_fp64(case, name, qkv, table, gout, device, label):
    want = reference(case, qkv, table, gout)
    floor = [rel_dist(g.double().cpu().numpy(), w.numpy())
             for g, w in zip(run(case, qkv, table, gout, device, torch_path=True), want)]
    got = run(case, qkv, table, gout, device)
    bad = []
    for k, g, w, f in zip(NAMES, got, want, floor):
        assert g.dtype == (torch.float32 if k == "dtable" else DTYPES[name]) and g.shape == w.shape, k
        assert torch.isfinite(g).all(), (label, name, k)
        d = rel_dist(g.double().cpu().numpy(), w.numpy())
        b = bound_of(name, f)
        print(f"SWEEP {label} {name} {k}: distance {d:.3e} floor {f:.3e} bound {b:.3e}")
        if not d <= b:
            bad.append((k, d, f, b))
    assert not bad, (label, name, bad)


@pytest.mark.parametrize("case,name", [(c, n) for c in CASES for n in dtypes_of(c)],
                         ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_matches_fp64(device, case, name):
    qkv, table, gout = make_inputs(case, DTYPES[name])
    check_against_fp64(case, name, qkv, table, gout, device, case_id(case))


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", TAIL_CASES, ids=case_id)
def test_tail_keys_stay_out(device, case, name):
    """q, k and v of the window's last token are 1e4.  The tail slots N .. NP-1 of the kernels' token tables repeat
    that token's entry and are kept out by a -inf penalty: a tail key that leaked into a softmax, or a tail row into
    dK / dV, would come with this token's magnitude.  One window (window_attn_cases.TAIL_CASES says why).  In fp16
    the torch path's own fp16 matmul overflows at these values: its floor is NaN and tol() stays at 1e-3."""
    qkv, table, gout = tail_inputs(case, DTYPES[name])
    check_against_fp64(case, name, qkv, table, gout, device, "tail-" + case_id(case))


def test_noncontiguous_qkv_and_gout(device):
    """qkv as a channel slice of a wider tensor and gout as a transposed view: bit for bit the contiguous run."""
    case = SWEEP6
    qkv, table, gout = make_inputs(case, torch.float16)
    want = run(case, qkv, table, gout, device)
    wide = torch.zeros(*qkv.shape[:3], qkv.shape[3] + 40, dtype=qkv.dtype, device=device)
    wide[..., 8:8 + qkv.shape[3]] = qkv.to(device)
    q_view = wide[..., 8:8 + qkv.shape[3]].detach().requires_grad_()
    g_view = gout.to(device).transpose(1, 2).contiguous().transpose(1, 2)
    assert not q_view.is_contiguous() and not g_view.is_contiguous()
    from bm2f_amd import window_attention
    t = table.to(device).requires_grad_()
    out = window_attention(q_view, t, case.nH, case.ws, case.shift)
    out.backward(g_view)
    assert q_view.grad.shape == q_view.shape
    for k, g, w in zip(NAMES, (out.detach(), q_view.grad, t.grad), want):
        assert torch.equal(g, w), k


def test_bf16_bias_table(device):
    """A bf16 table is read as its fp32 values, and its gradient comes back in bf16: the fp32 result rounded."""
    case = SWEEP6
    qkv, table, gout = make_inputs(case, torch.float32)
    table16 = table.bfloat16()
    want = run(case, qkv, table16.float(), gout, device)
    got = run(case, qkv, table16, gout, device)
    assert got[2].dtype == torch.bfloat16
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2].bfloat16())


@pytest.mark.parametrize("case", [SWEEP6, SWEEP3], ids=case_id)
def test_bitwise_repeatable(device, case):
    qkv, table, gout = make_inputs(case, torch.float16)
    first = run(case, qkv, table, gout, device)
    second = run(case, qkv, table, gout, device)
    for k, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), k
