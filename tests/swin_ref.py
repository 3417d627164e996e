"""Functional torch restatement of the Swin block (fp64-capable), for shapes the fixtures do not hold, plus the
loader of the ``tests/golden/swin*.npz`` fixtures.

Written apart from ``bm2f_amd/swin.py`` on purpose: the shift mask comes from explicit slices over a label image and
the windows from index lists, not from the arithmetic the package uses.  ``tests/test_swin_cpu.py`` pins both functions
to the reference's results stored in the fixtures.
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(prefix):
    """All arrays of tests/golden/<prefix>*.npz; ``name__pK`` parts are joined along axis 0."""
    raw = {}
    files = sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))
    if not files:
        raise FileNotFoundError(f"no fixture {prefix}*.npz")
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            for k in z.files:
                raw[k] = z[k]
    out, parts = {}, {}
    for k, v in raw.items():
        if "__p" in k:
            name, idx = k.rsplit("__p", 1)
            parts.setdefault(name, {})[int(idx)] = v
        else:
            out[k] = v
    for name, d in parts.items():
        out[name] = np.concatenate([d[i] for i in range(len(d))], axis=0)
    return out


def _window_pixels(Hp, Wp, ws, shift):
    """(nW, N) int64: flat pixel index (row * Wp + col, unshifted map) of every token of every window."""
    idx = []
    for wy in range(Hp // ws):
        for wx in range(Wp // ws):
            idx.append([((wy * ws + ty + shift) % Hp) * Wp + (wx * ws + tx + shift) % Wp
                        for ty in range(ws) for tx in range(ws)])
    return torch.tensor(idx, dtype=torch.int64)


def _window_labels(Hp, Wp, ws, shift):
    """(nW, N) labels of the shifted map's nine regions, painted with slices."""
    img = torch.zeros(Hp, Wp, dtype=torch.int64)
    cuts = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    n = 0
    for hs in cuts:
        for wsl in cuts:
            img[hs, wsl] = n
            n += 1
    lab = []
    for wy in range(Hp // ws):
        for wx in range(Wp // ws):
            lab.append(img[wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws].reshape(-1))
    return torch.stack(lab)


def window_attention_ref(qkv, table, num_heads, ws, shift, scale=None, return_attn=False):
    """qkv (B, Hp, Wp, 3C), table ((2ws-1)^2, nH) -> (B, Hp, Wp, C); any float dtype, differentiable."""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    D = C // num_heads
    scale = D ** -0.5 if scale is None else scale
    pix = _window_pixels(Hp, Wp, ws, shift)                     # (nW, N)
    nW, N = pix.shape
    win = qkv.reshape(B, Hp * Wp, 3, num_heads, D)[:, pix]       # (B, nW, N, 3, nH, D)
    q, k, v = (win[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))     # (B, nW, nH, N, D)
    s = torch.einsum("bwhid,bwhjd->bwhij", q * scale, k)
    ty, tx = torch.arange(N) // ws, torch.arange(N) % ws
    rel = (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + tx[:, None] - tx[None, :] + ws - 1
    s = s + table[rel].permute(2, 0, 1)
    if shift > 0:
        lab = _window_labels(Hp, Wp, ws, shift)
        s = s + torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0).to(s.dtype)[None, :, None]
    p = torch.softmax(s, dim=-1)
    if return_attn:
        return p, pix
    o = torch.einsum("bwhij,bwhjd->bwihd", p, v).reshape(B, nW * N, C)
    inv = torch.empty(nW * N, dtype=torch.int64)
    inv[pix.reshape(-1)] = torch.arange(nW * N)
    return o[:, inv].reshape(B, Hp, Wp, C)


def block_ref(x, H, W, sd, num_heads, ws, shift, prefix=""):
    """One Swin block on x (B, H*W, C) with the parameters ``sd[prefix + name]`` (state-dict names of the block)."""
    p = lambda n: sd[prefix + n].to(x.dtype)   # noqa: E731
    B, L, C = x.shape
    y = F.layer_norm(x, (C,), p("norm1.weight"), p("norm1.bias")).reshape(B, H, W, C)
    pb, pr = (ws - H % ws) % ws, (ws - W % ws) % ws
    y = F.pad(y, (0, 0, 0, pr, 0, pb))
    qkv = F.linear(y, p("attn.qkv.weight"), p("attn.qkv.bias"))
    a = window_attention_ref(qkv, p("attn.relative_position_bias_table"), num_heads, ws, shift)
    a = F.linear(a, p("attn.proj.weight"), p("attn.proj.bias"))[:, :H, :W].reshape(B, L, C)
    x = x + a
    z = F.layer_norm(x, (C,), p("norm2.weight"), p("norm2.bias"))
    z = F.linear(F.gelu(F.linear(z, p("mlp.fc1.weight"), p("mlp.fc1.bias"))), p("mlp.fc2.weight"), p("mlp.fc2.bias"))
    return x + z


def rel_dist(got, want):
    """max |got - want| / max |want| in fp64."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
