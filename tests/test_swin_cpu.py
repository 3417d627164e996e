"""Swin backbone without a GPU: the torch path of window_attention and the modules against the reference's results
(tests/golden/swin_*.npz, gen_swin_golden.py), state-dict parity, the registry and the C-ABI argument refusals."""
import ctypes
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from filler import fill_module
from swin_ref import block_ref, load_golden, rel_dist, window_attention_ref

OP_CASES = "abcdef"
TINY = dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0)


def tol(floor):
    """The project's standing rule: 1e-3 of the tensor's max, or twice the reference's own fp32 error if larger."""
    return max(1e-3, 2.0 * float(floor))


@pytest.fixture(scope="module")
def tiny_fx():
    return load_golden("swin_tiny")


def _op_inputs(fx, dtype):
    B, nH, Hp, Wp, ws, shift = (int(v) for v in fx["meta"])
    qkv = torch.from_numpy(fx["qkv"]).to(dtype).requires_grad_()
    table = torch.from_numpy(fx["table"]).to(dtype).requires_grad_()
    return qkv, table, torch.from_numpy(fx["gout"]).to(dtype), nH, ws, shift


@pytest.mark.parametrize("case", OP_CASES)
def test_window_attention_torch_path_matches_reference(case):
    from bm2f_amd import window_attention
    fx = load_golden(f"swin_op_{case}")
    for dtype, bound in ((torch.float64, lambda f: 1e-12), (torch.float32, tol)):
        qkv, table, gout, nH, ws, shift = _op_inputs(fx, dtype)
        out = window_attention(qkv, table, nH, ws, shift)
        out.backward(gout)
        for name, got, k in (("out", out.detach(), 0), ("dqkv", qkv.grad, 1), ("dtable", table.grad, 2)):
            d = rel_dist(got.numpy(), fx[name])
            assert d <= bound(fx["floor"][k]), (case, dtype, name, d)


@pytest.mark.parametrize("case", OP_CASES)
def test_swin_ref_op_pinned_to_fixture(case):
    fx = load_golden(f"swin_op_{case}")
    qkv, table, gout, nH, ws, shift = _op_inputs(fx, torch.float64)
    out = window_attention_ref(qkv, table, nH, ws, shift)
    out.backward(gout)
    assert rel_dist(out.detach().numpy(), fx["out"]) < 1e-12
    assert rel_dist(qkv.grad.numpy(), fx["dqkv"]) < 1e-12
    assert rel_dist(table.grad.numpy(), fx["dtable"]) < 1e-12


def test_swin_ref_block_pinned_to_fixture():
    from bm2f_amd.swin import SwinTransformerBlock
    fx = load_golden("swin_block")
    B, H, W, dim, nH, ws, shift = (int(v) for v in fx["meta"])
    blk = fill_module(SwinTransformerBlock(dim=dim, num_heads=nH, window_size=ws, shift_size=shift)).double()
    x = torch.from_numpy(fx["x"]).double()
    y = block_ref(x, H, W, blk.state_dict(), nH, ws, shift)
    assert rel_dist(y.numpy(), fx["y"]) < 1e-12
    # and the package's block on the CPU, fp64 and fp32
    blk.H, blk.W = H, W
    assert rel_dist(blk(x).detach().numpy(), fx["y"]) < 1e-12
    blk32 = blk.float()
    assert rel_dist(blk32(x.float()).detach().numpy(), fx["y"]) <= tol(fx["floor"][0])


def test_masked_pairs_and_tail_free_rows_cpu():
    """The -100 is added, not -inf: other-region keys keep a probability at the e^-100 level."""
    from bm2f_amd.swin import window_attention_torch
    fx = load_golden("swin_op_b")
    qkv, table, _, nH, ws, shift = _op_inputs(fx, torch.float64)
    p = window_attention_torch(qkv.detach(), table.detach(), nH, ws, shift, return_attn=True)
    p_ref, _ = window_attention_ref(qkv.detach(), table.detach(), nH, ws, shift, return_attn=True)
    assert torch.allclose(p, p_ref, rtol=1e-10, atol=1e-300)
    assert (p > 0).all()


def run_tiny(model, fx, dtype, device="cpu", autocast=None):
    x = torch.from_numpy(fx["x"]).to(device=device, dtype=dtype).requires_grad_()
    if autocast is not None:
        with torch.autocast(device_type=torch.device(device).type, dtype=autocast):
            feats = model(x)
    else:
        feats = model(x)
    loss = sum((feats[k].to(dtype) * torch.from_numpy(fx[f"g_{k}"]).to(device=device, dtype=dtype)).mean()
               for k in sorted(feats))
    loss.backward()
    return feats, x.grad


def check_tiny(model, feats, dx, fx, floor_scale=1.0, grads=True):
    for k in ("res2", "res3", "res4", "res5"):
        d = rel_dist(feats[k].detach().double().cpu().numpy(), fx[k])
        assert d <= tol(fx[f"{k}_floor"][0]) * floor_scale, (k, d)
    if not grads:
        return
    d = rel_dist(dx.double().cpu().numpy(), fx["dx"])
    assert d <= tol(fx["dx_floor"][0]), ("dx", d)
    params = dict(model.named_parameters())
    n_full = 0
    for key in fx:
        if key.startswith("grad:"):
            name = key[5:]
            d = rel_dist(params[name].grad.double().cpu().numpy(), fx[key])
            assert d <= tol(fx["grad_floor:" + name][0]), (name, d)
            n_full += 1
    assert n_full >= 8 * 2 + 8 * 2   # tables, qkv biases and the blocks' two norms
    for name, row in zip(fx["grad_sum_names"], fx["grad_sums"]):
        g = params[str(name)].grad.double()
        # the sum is compared on the scale of the absolute sum (a signed sum near zero carries no relative meaning);
        # floor: the reference's own fp32 sum against its fp64 sum
        floor = abs(row[2] - row[0]) / max(row[1], 1e-300)
        assert abs(float(g.sum()) - row[0]) <= tol(floor) * row[1], name
        assert abs(float(g.abs().sum()) - row[1]) <= tol(abs(row[3] - row[1]) / max(row[1], 1e-300)) * row[1], name


def test_tiny_backbone_cpu(tiny_fx):
    from bm2f_amd import SwinTransformer
    model = fill_module(SwinTransformer(**TINY)).train()
    feats, dx = run_tiny(model, tiny_fx, torch.float32)
    assert [tuple(feats[k].shape[-2:]) for k in sorted(feats)] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    check_tiny(model, feats, dx, tiny_fx)


def test_state_dict_matches_reference_and_loads_strict(tiny_fx):
    from bm2f_amd import SwinTransformer
    model = SwinTransformer(**TINY)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in tiny_fx["state_keys"]]
    for v, shape in zip(sd.values(), tiny_fx["state_shapes"]):
        assert list(v.shape) == [int(s) for s in shape if s >= 0]
    idx = sd["layers.0.blocks.0.attn.relative_position_index"]
    assert idx.dtype == torch.int64 and idx[0, 0] == 84 and idx[0, 48] == 0 and idx[48, 0] == 168
    # a checkpoint with exactly the reference's keys loads strictly, buffers included
    ckpt = {str(k): torch.zeros([int(s) for s in shape if s >= 0], dtype=sd[str(k)].dtype)
            for k, shape in zip(tiny_fx["state_keys"], tiny_fx["state_shapes"])}
    res = SwinTransformer(**TINY).load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def _cfg(**over):
    s = dict(PRETRAIN_IMG_SIZE=224, PATCH_SIZE=4, EMBED_DIM=32, DEPTHS=[2, 2, 2, 2], NUM_HEADS=[1, 2, 4, 8],
             WINDOW_SIZE=7, MLP_RATIO=4.0, QKV_BIAS=True, QK_SCALE=None, DROP_RATE=0.0, ATTN_DROP_RATE=0.0,
             DROP_PATH_RATE=0.3, APE=False, PATCH_NORM=True, OUT_FEATURES=["res3", "res5"], USE_CHECKPOINT=False)
    s.update(over)
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(SWIN=types.SimpleNamespace(**s)))


def test_registry_lookup_and_d2_surface():
    from bm2f_amd import D2SwinTransformer, registry
    cls = registry.BACKBONE_REGISTRY.get("D2SwinTransformer")
    assert cls is D2SwinTransformer
    m = cls(_cfg(), None)
    assert m.size_divisibility == 32
    shp = m.output_shape()
    assert sorted(shp) == ["res3", "res5"]
    assert (shp["res3"].channels, shp["res3"].stride, shp["res5"].channels, shp["res5"].stride) == (64, 8, 256, 32)
    out = m.eval()(torch.zeros(1, 3, 32, 64))
    assert sorted(out) == ["res3", "res5"] and out["res5"].shape == (1, 256, 1, 2)
    # stochastic depth is restated in torch: rates rise linearly over the blocks, identity in eval
    from bm2f_amd.swin import DropPath
    rates = [b.drop_path.drop_prob for layer in m.layers for b in layer.blocks if isinstance(b.drop_path, DropPath)]
    assert len(rates) == 7 and abs(rates[-1] - 0.3) < 1e-6 and rates == sorted(rates)
    dp = DropPath(0.5).train()
    torch.manual_seed(0)
    y = dp(torch.ones(64, 3, 2))
    per = y.flatten(1)
    assert ((per == 0).all(1) | (per == 2).all(1)).all() and 0 < int((per[:, 0] == 0).sum()) < 64
    assert torch.equal(dp.eval()(torch.ones(4, 2)), torch.ones(4, 2))
    # use_checkpoint gives the same result
    a = cls(_cfg(DROP_PATH_RATE=0.0), None)
    b = cls(_cfg(DROP_PATH_RATE=0.0, USE_CHECKPOINT=True), None)
    b.load_state_dict(a.state_dict())
    x = torch.randn(1, 3, 32, 32, requires_grad=True)
    assert torch.allclose(a(x)["res5"], b(x)["res5"], atol=1e-6)


_ORDER = """
import sys, types
from torch import nn
sys.path.insert(0, {root!r})
class Registry:                       # raises on a duplicate name, as detectron2's does
    def __init__(self, name): self._name, self._obj_map = name, {{}}
    def register(self, obj=None):
        if obj is None: return lambda o: self.register(o)
        assert obj.__name__ not in self._obj_map, "already registered"
        self._obj_map[obj.__name__] = obj
        return obj
    def get(self, name): return self._obj_map[name]
# a host framework that owns the backbone registry exists before bm2f_amd is first imported
host = types.ModuleType("detectron2.modeling")
host.BACKBONE_REGISTRY, host.Backbone = Registry("BACKBONE"), nn.Module
sys.modules["detectron2"] = types.ModuleType("detectron2")
sys.modules["detectron2.modeling"] = host
class D2SwinTransformer(nn.Module): pass      # the host's own class of the same name
assert not any(m == "bm2f_amd" or m.startswith("bm2f_amd.") for m in sys.modules)
{body}
import bm2f_amd.registry as r
import bm2f_amd.swin as s
assert r.BACKBONE_REGISTRY is host.BACKBONE_REGISTRY
assert host.BACKBONE_REGISTRY.get("D2SwinTransformer") is s.D2SwinTransformer
assert issubclass(s.D2SwinTransformer, host.Backbone)
print("ORDER_OK")
"""


@pytest.mark.parametrize("order", ["other_first", "bm2f_first"])
def test_install_both_import_orders(order):
    """The host's registry (a stand-in seeded into sys.modules before the first bm2f import) ends up holding bm2f's
    D2SwinTransformer in either order.  other_first: the host's class is registered when bm2f_amd is imported, and the
    import itself replaces it instead of raising.  bm2f_first: bm2f registers, the host then puts its own class under
    the name, and install() puts bm2f's back."""
    if order == "other_first":
        body = ("host.BACKBONE_REGISTRY.register(D2SwinTransformer)\n"
                "import bm2f_amd\n")
    else:
        body = ("import bm2f_amd\n"
                "import bm2f_amd.swin\n"
                "assert host.BACKBONE_REGISTRY.get('D2SwinTransformer') is bm2f_amd.swin.D2SwinTransformer\n"
                "host.BACKBONE_REGISTRY._obj_map['D2SwinTransformer'] = D2SwinTransformer\n"
                "import bm2f_amd.registry\n"
                "bm2f_amd.registry.install()\n")
    p = subprocess.run([sys.executable, "-c", _ORDER.format(root=ROOT, body=body)], capture_output=True, text=True)
    assert p.returncode == 0 and "ORDER_OK" in p.stdout, p.stderr[-2000:]


def test_frozen_stages_and_attn_drop():
    from bm2f_amd import SwinTransformer
    m = SwinTransformer(frozen_stages=2, **TINY).train()
    assert not m.patch_embed.training and not any(p.requires_grad for p in m.patch_embed.parameters())
    assert not m.layers[0].training and not any(p.requires_grad for p in m.layers[0].parameters())
    assert m.layers[1].training and all(p.requires_grad for p in m.layers[1].parameters())
    assert m.train() is m
    with pytest.raises(NotImplementedError):
        SwinTransformer(attn_drop_rate=0.1, **TINY)


def test_window_attention_argument_errors():
    from bm2f_amd import window_attention
    qkv, table = torch.zeros(1, 14, 14, 96), torch.zeros(169, 1)
    with pytest.raises(ValueError):
        window_attention(qkv, table, 1, 5, 0)        # 14 % 5
    with pytest.raises(ValueError):
        window_attention(qkv, table, 1, 7, 7)        # shift == ws
    with pytest.raises(ValueError):
        window_attention(qkv, torch.zeros(168, 1), 1, 7, 0)


def test_capi_refusals_without_gpu():
    from bm2f_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    f = ctypes.c_float(0.25)
    nb = ctypes.c_int64(0)

    def fwd(dtype=0, heads=2, hd=32, hp=14, wp=21, ws=7, shift=3, qkv=p):
        return lib.m2f_window_attn_fwd(dtype, qkv, p, 2, heads, hd, hp, wp, ws, shift, f, p, p, None)

    def bwd(hd=32, hp=14, wp=21, ws=7, shift=3, work=p, nbytes=1 << 40, dq=p):
        return lib.m2f_window_attn_bwd(0, p, p, p, p, 2, 2, hd, hp, wp, ws, shift, f, dq, p, work,
                                       ctypes.c_int64(nbytes), None)

    assert fwd(qkv=None) == 1 and b"null" in lib.m2f_last_error()
    assert bwd(dq=None) == 1 and b"null" in lib.m2f_last_error()
    assert bwd(work=None) == 1 and b"null" in lib.m2f_last_error()
    for fn in (fwd, bwd):
        assert fn(ws=13, hp=13, wp=13) == 3 and b"window size" in lib.m2f_last_error()
        assert fn(ws=1) == 3 and b"window size" in lib.m2f_last_error()
        assert fn(hd=64) == 3 and b"head_dim" in lib.m2f_last_error()
        assert fn(hp=15) == 1 and b"multiple" in lib.m2f_last_error()
        assert fn(wp=20) == 1 and b"multiple" in lib.m2f_last_error()
        assert fn(shift=7) == 1 and b"shift" in lib.m2f_last_error()
        assert fn(shift=-1) == 1 and b"shift" in lib.m2f_last_error()
    assert fwd(dtype=9) == 3 and b"dtype" in lib.m2f_last_error()
    assert lib.m2f_window_attn_workspace(2, 2, 14, 21, 7, ctypes.byref(nb)) == 0
    assert nb.value == 2 * 6 * 2 * 169 * 4
    assert bwd(nbytes=nb.value - 4) == 1 and b"workspace" in lib.m2f_last_error()
    assert lib.m2f_window_attn_workspace(2, 2, 14, 21, 7, None) == 1
    assert lib.m2f_window_attn_workspace(2, 2, 14, 20, 7, ctypes.byref(nb)) == 1
    # a success clears the thread's message
    assert lib.m2f_window_attn_workspace(1, 1, 7, 7, 7, ctypes.byref(nb)) == 0 and lib.m2f_last_error() == b""
