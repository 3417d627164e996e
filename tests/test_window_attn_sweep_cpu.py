"""The shifted-window attention sweep without a GPU (cases: tests/window_attn_cases.py).

1. tests/swin_ref.window_attention_ref (slices over a label image, index lists) and bm2f_amd.swin.window_attention_torch
   (roll, partition, analytic regions) were written apart and are pinned to the reference's fixtures at ws 5, 7 and 12
   only; here they agree in fp64 to 1e-12 at every window size, shift, scale and window count of the sweep.
2. The sweep's inputs discriminate: a bias table rolled by one row or reversed (the query / key swap of the relative
   index), a shift off by one and a scale of 0.2 each move the fp64 output by at least 0.05 of its max at every
   ws 2 .. 12.  The loosest bound the GPU test applies is twice the bf16 torch-path floor, about 0.024.
3. ``window_attention`` on CPU tensors runs the torch path and returns what it returns.
"""
import pytest
import torch

from swin_ref import rel_dist, window_attention_ref
from window_attn_cases import (CASES, DTYPES, SWEEP_SHIFTED, TAIL_CASES, case_id, make_inputs, reference, scale_of,
                               tail_inputs, tiles_of)

SENSITIVITY = 0.05


def test_case_table_reaches_every_tile_count():
    assert {tiles_of(c.ws) for c in CASES} == {1, 2, 3, 4, 6, 7, 8, 9}
    assert {c.ws for c in CASES if c.group == "sweep"} == set(range(2, 13))
    assert {(c.ws, c.shift) for c in CASES} >= {(ws, s) for ws in (6, 8, 9, 11) for s in (1, ws - 1)} | {(3, 1), (3, 2)}
    assert {c.B * c.windows[0] * c.windows[1] for c in CASES} == {1, 3, 9, 12}
    assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_fp64_restatements_agree(case):
    from bm2f_amd.swin import window_attention_torch
    qkv, table, gout = make_inputs(case)
    want = reference(case, qkv, table, gout)
    got = reference(case, qkv, table, gout, fn=window_attention_torch)
    for name, g, w in zip(("out", "dqkv", "dtable"), got, want):
        assert torch.isfinite(w).all(), name
        d = rel_dist(g.numpy(), w.numpy())
        assert d <= 1e-12, (name, d)


@pytest.mark.parametrize("case", SWEEP_SHIFTED, ids=case_id)
def test_inputs_discriminate(case):
    qkv, table, _ = make_inputs(case)
    ws, shift, nH = case.ws, case.shift, case.nH
    base = window_attention_ref(qkv, table, nH, ws, shift, scale_of(case)).numpy()
    mutants = {
        "table rolled by one": window_attention_ref(qkv, torch.roll(table, 1, 0), nH, ws, shift, scale_of(case)),
        "table reversed": window_attention_ref(qkv, table.flip(0), nH, ws, shift, scale_of(case)),
        "scale 0.2": window_attention_ref(qkv, table, nH, ws, shift, 0.2),
    }
    if ws > 2:
        mutants["shift off by one"] = window_attention_ref(qkv, table, nH, ws, shift + 1, scale_of(case))
    for name, out in mutants.items():
        d = rel_dist(out.numpy(), base)
        print(f"{case_id(case)} {name}: moves the output by {d:.3f} of its max")
        assert d >= SENSITIVITY, (name, d)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", TAIL_CASES, ids=case_id)
def test_tail_isolation_inputs_are_well_conditioned(case, name):
    """With a token of 1e4 a query row whose score against it nearly ties with the rest makes the gradients turn on the
    last bits of the inputs (window_attn_cases.TAIL_CASES).  The inputs of the GPU test hold no such row: moving q, k
    and v by half an fp32 ulp moves the fp64 result by less than 1e-6 of its max, half of the smallest fp32 bound, and
    every result fits the fp16 range."""
    qkv, table, gout = tail_inputs(case, DTYPES[name])
    want = reference(case, qkv, table, gout)
    g = torch.Generator().manual_seed(1)
    sign = torch.randint(0, 2, qkv.shape, generator=g).double() * 2 - 1
    moved = reference(case, qkv.double() * (1 + sign * 2.0 ** -24), table, gout)
    assert float(want[0].abs().max()) > 9e3        # the filled token's v reaches the output
    for k, m, w in zip(("out", "dqkv", "dtable"), moved, want):
        assert float(w.abs().max()) < 6e4, k
        d = rel_dist(m.numpy(), w.numpy())
        assert d < 1e-6, (k, d)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_tensors_take_the_torch_path(case, monkeypatch):
    from bm2f_amd import swin

    def no_device_path(*a, **k):
        raise AssertionError("CPU tensors were sent to the library")

    monkeypatch.setattr(swin._WindowAttention, "apply", no_device_path)
    qkv, table, gout = make_inputs(case, torch.float32)
    runs = []
    for fn in (swin.window_attention, swin.window_attention_torch):
        q, t = qkv.clone().requires_grad_(), table.clone().requires_grad_()
        out = fn(q, t, case.nH, case.ws, case.shift, case.scale)
        out.backward(gout)
        runs.append((out.detach(), q.grad, t.grad))
    (out_a, dq_a, dt_a), (out_b, dq_b, dt_b) = runs
    assert torch.equal(out_a, out_b) and torch.equal(dq_a, dq_b)
    # the table gradient is torch's index_put accumulation, whose order over threads is not fixed: two runs of the
    # same function differ in the last bits.  A bin sums at most N * windows < 2000 fp32 terms, so a reordering moves
    # it by a few 1e-6 of the largest at the most
    assert rel_dist(dt_a.numpy(), dt_b.numpy()) <= 1e-5
