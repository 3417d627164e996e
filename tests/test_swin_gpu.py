"""Shifted-window attention kernels (csrc/window_attn.hip) and the Swin modules on the GPU, against the reference's fp64
results in tests/golden/swin_*.npz and, for shapes the fixtures do not hold, tests/swin_ref.py in fp64.

op case   B nH  grid   ws shift  reaches
   a      2  2  14x21   7   0    tail tile (49 -> 64), no mask
   b      2  2  14x21   7   3    all nine regions, wrap-around rows and columns
   c      1  3   7x7    7   3    one window = whole map, empty first slice
   d      2  1  24x36  12   6    9 full tiles, regions
   e      1  2  24x12  12   0    one window column
   f      1  2  10x15   5   2    odd ws, N = 25 -> 32

These reach three of the kernels' eight tile counts (4, 9 and 2 tiles of 16 tokens).  tests/test_window_attn_sweep_gpu.py
runs every window size 2 .. 12, shifts other than ws // 2, other scales and few windows, with a tighter fp32 bound.

Tolerance: every tensor within max(1e-3, 2 x floor) of its max, where the floor is the torch
path's own distance from fp64 in the same I/O precision (fp32 softmax in every precision, as autocast runs it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from filler import fill_module
from swin_ref import _window_labels, _window_pixels, block_ref, load_golden, rel_dist
from test_swin_cpu import TINY, check_tiny, run_tiny, tol

pytestmark = pytest.mark.gpu

OP_CASES = "abcdef"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
_cache = {}


def fixture_of(case):
    if case not in _cache:
        _cache[case] = load_golden(f"swin_op_{case}")
    return _cache[case]


def run_op(fx, dtype, device, torch_path=False):
    from bm2f_amd import window_attention
    from bm2f_amd.swin import window_attention_torch
    _, nH, _, _, ws, shift = (int(v) for v in fx["meta"])
    qkv = torch.from_numpy(fx["qkv"]).to(device, dtype).requires_grad_()
    table = torch.from_numpy(fx["table"]).to(device).requires_grad_()
    gout = torch.from_numpy(fx["gout"]).to(device, dtype)
    fn = window_attention_torch if torch_path else window_attention
    out = fn(qkv, table, nH, ws, shift)
    out.backward(gout)
    return out.detach(), qkv.grad, table.grad


def floors(case, name, device):
    """Distance of the torch path from the fp64 fixture in the given I/O precision: out, dqkv, dtable."""
    key = ("floor", case, name)
    if key not in _cache:
        fx = fixture_of(case)
        got = run_op(fx, DTYPES[name], device, torch_path=True)
        _cache[key] = [rel_dist(g.double().cpu().numpy(), fx[k]) for g, k in zip(got, ("out", "dqkv", "dtable"))]
    return _cache[key]


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", OP_CASES)
def test_window_attention_matches_fp64(device, case, name):
    fx = fixture_of(case)
    got = run_op(fx, DTYPES[name], device)
    fl = floors(case, name, device)
    for g, k, f in zip(got, ("out", "dqkv", "dtable"), fl):
        d = rel_dist(g.double().cpu().numpy(), fx[k])
        print(f"case {case} {name} {k}: distance {d:.3e}, torch-path floor {f:.3e}")
        assert d <= tol(f), (case, name, k, d, f)


def test_masked_pairs_weigh_exp_minus_100(device):
    """v made a one-hot of each key's region label: channel r of a query's output is then that row's probability mass
    on region r.  The mass on the other regions must be at the e^-100 level, not merely small."""
    from bm2f_amd import window_attention
    fx = fixture_of("b")
    B, nH, Hp, Wp, ws, shift = (int(v) for v in fx["meta"])
    C = nH * 32
    qkv = torch.from_numpy(fx["qkv"]).clone()
    lab_img = torch.empty(Hp * Wp, dtype=torch.int64)
    lab_img[_window_pixels(Hp, Wp, ws, shift).reshape(-1)] = _window_labels(Hp, Wp, ws, shift).reshape(-1)
    onehot = torch.nn.functional.one_hot(lab_img, 32).float().reshape(1, Hp, Wp, 1, 32)
    qkv[..., 2 * C:] = onehot.expand(B, Hp, Wp, nH, 32).reshape(B, Hp, Wp, C)
    out = window_attention(qkv.to(device), torch.from_numpy(fx["table"]).to(device), nH, ws, shift)
    mass = out.cpu().reshape(B, Hp * Wp, nH, 32)
    own = mass.gather(-1, lab_img.view(1, -1, 1, 1).expand(B, -1, nH, 1))[..., 0]
    other = mass.sum(-1) - own
    # windows on the wrap-around hold several regions: those rows exist and are the ones that matter
    assert len(torch.unique(lab_img)) == 9
    assert float((own - 1).abs().max()) < 1e-5
    assert float(mass[..., 9:].abs().max()) == 0.0
    other_direct = mass.clone()
    other_direct.scatter_(-1, lab_img.view(1, -1, 1, 1).expand(B, -1, nH, 1), 0.0)
    assert float(other_direct.max()) < 1e-30, float(other_direct.max())
    assert float(other_direct.min()) >= 0.0 and float(other.abs().max()) < 1e-5


@pytest.mark.parametrize("name", ["fp32", "fp16"])
def test_bitwise_repeatable(device, name):
    fx = fixture_of("b")
    first = run_op(fx, DTYPES[name], device)
    second = run_op(fx, DTYPES[name], device)
    for a, b, k in zip(first, second, ("out", "dqkv", "dtable")):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", ["fp16", "fp32"])
def test_graph_capture_no_memset(device, name):
    cmd = [sys.executable, os.path.join(ROOT, "tests", "swin_graph_child.py"), "--dtype", name]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "SWIN_GRAPH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_unsupported_shapes_raise_on_device(device):
    from bm2f_amd import _native, window_attention
    with pytest.raises(_native.NativeError, match="head_dim"):
        window_attention(torch.zeros(1, 7, 7, 3 * 64, device=device), torch.zeros(169, 1, device=device), 1, 7, 0)
    with pytest.raises(_native.NativeError, match="window size"):
        window_attention(torch.zeros(1, 13, 13, 96, device=device), torch.zeros(625, 1, device=device), 1, 13, 0)
    with pytest.raises(TypeError):
        window_attention(torch.zeros(1, 7, 7, 96, device=device, dtype=torch.float64),
                         torch.zeros(169, 1, device=device), 1, 7, 0)


def test_needs_input_grad_and_no_double_backward(device):
    from bm2f_amd import window_attention
    fx = fixture_of("f")
    _, nH, _, _, ws, shift = (int(v) for v in fx["meta"])
    qkv = torch.from_numpy(fx["qkv"]).to(device).requires_grad_()
    table = torch.from_numpy(fx["table"]).to(device)          # no gradient asked for the table
    gout = torch.from_numpy(fx["gout"]).to(device).requires_grad_()   # a differentiable upstream gradient
    out = window_attention(qkv, table, nH, ws, shift)
    (dq,) = torch.autograd.grad(out, qkv, gout, create_graph=True)
    assert table.grad is None and rel_dist(dq.detach().cpu().numpy(), fx["dqkv"]) < 1e-3
    with pytest.raises(RuntimeError, match="once_differentiable"):
        dq.sum().backward()


@pytest.fixture(scope="module")
def tiny_fx():
    return load_golden("swin_tiny")


def test_tiny_backbone_fp32(device, tiny_fx):
    from bm2f_amd import SwinTransformer
    model = fill_module(SwinTransformer(**TINY)).to(device).train()
    feats, dx = run_tiny(model, tiny_fx, torch.float32, device=device)
    check_tiny(model, feats, dx, tiny_fx)


def test_tiny_backbone_autocast_fp16(device, tiny_fx):
    """Features under autocast against fp64, the floor being the torch path under the same autocast."""
    from bm2f_amd import SwinTransformer, swin
    model = fill_module(SwinTransformer(**TINY)).to(device).train()
    x = torch.from_numpy(tiny_fx["x"]).to(device)
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        feats = model(x)
        real = swin.window_attention
        swin.window_attention = lambda q, t, nH, ws, shift, scale=None: swin.window_attention_torch(q, t, nH, ws, shift,
                                                                                                  scale)
        try:
            base = model(x)
        finally:
            swin.window_attention = real
    for k in sorted(feats):
        d = rel_dist(feats[k].detach().double().cpu().numpy(), tiny_fx[k])
        f = rel_dist(base[k].detach().double().cpu().numpy(), tiny_fx[k])
        print(f"{k}: distance {d:.3e}, torch-path floor {f:.3e}")
        assert d <= tol(f), (k, d, f)


def test_padded_block_against_swin_ref(device):
    """13 x 17 at ws 7: padded to 14 x 21 after norm1, so the padded tokens are keys that carry only the qkv bias."""
    from bm2f_amd.swin import SwinTransformerBlock
    B, H, W, dim, nH, ws, shift = 2, 13, 17, 64, 2, 7, 3
    blk = fill_module(SwinTransformerBlock(dim=dim, num_heads=nH, window_size=ws, shift_size=shift))
    blk.H, blk.W = H, W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H * W, dim, generator=g)
    gy = torch.randn(B, H * W, dim, generator=g)
    sd64 = {k: v.double().requires_grad_() if v.is_floating_point() else v for k, v in blk.state_dict().items()}
    x64 = x.double().requires_grad_()
    y64 = block_ref(x64, H, W, sd64, nH, ws, shift)
    y64.backward(gy.double())
    # floor: the same block in fp32 on the CPU (torch path)
    x32 = x.clone().requires_grad_()
    y32 = blk(x32)
    y32.backward(gy)
    cpu = {"y": y32.detach(), "dx": x32.grad, **{k: p.grad.clone() for k, p in blk.named_parameters()}}
    blk.zero_grad()
    blk = blk.to(device)
    xd = x.to(device).requires_grad_()
    yd = blk(xd)
    yd.backward(gy.to(device))
    want = {"y": y64.detach(), "dx": x64.grad, **{k: sd64[k].grad for k, _ in blk.named_parameters()}}
    got = {"y": yd.detach(), "dx": xd.grad, **{k: p.grad for k, p in blk.named_parameters()}}
    for k in want:
        d = rel_dist(got[k].double().cpu().numpy(), want[k].numpy())
        f = rel_dist(cpu[k].double().numpy(), want[k].numpy())
        assert d <= tol(f), (k, d, f)
