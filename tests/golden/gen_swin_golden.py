"""Generate tests/golden/swin_*.npz by running the REFERENCE Swin backbone on the CPU (nothing of the reference is
copied: the fixtures hold inputs, results and name lists only).

    python tests/golden/gen_swin_golden.py --ref <reference checkout>

``mask2former/modeling/backbone/swin.py`` is imported in place, with this file's stand-ins for what it imports from
``timm`` (DropPath, to_2tuple, trunc_normal_) and ``detectron2`` (BACKBONE_REGISTRY, Backbone, ShapeSpec) when those
packages are not importable.

Three groups, every result computed by the reference in fp32 and in fp64 (the fp64 one is stored, with the reference's
own fp32-versus-fp64 distance per tensor, ``*_floor``: the tests' noise floor):

* ``swin_op_<case>``: the core between the qkv and proj linears.  The reference's own roll, ``window_partition``,
  ``WindowAttention.forward`` (its qkv replaced by a stub that hands over the partitioned qkv, its proj by the
  identity), ``window_reverse`` and roll, with the shift mask that ``BasicLayer.forward`` builds.  Stored: qkv, table,
  the upstream gradient, out, dqkv and the table gradient.
* ``swin_block``: one ``SwinTransformerBlock`` on a 13 x 17 map (padded to 14 x 21), which pins tests/swin_ref.py.
* ``swin_tiny``: a four-stage backbone (stage grids 16x24, 8x12, 4x6, 2x3 for ws 7: three padded, one window-sized)
  with ``filler.fill_module`` weights: res2..res5, and for the loss sum_k mean(res_k * g_k) the input gradient, the
  gradients of every relative_position_bias_table, qkv.bias and norm*.weight, and the sum / absolute sum of every
  other parameter's gradient; plus the state-dict key and shape list.

Arrays larger than a file may hold are split along axis 0 into ``name__p0, name__p1, ...`` (tests/swin_ref.py joins
them); every file stays under 1 MiB, with fixed timestamps and sorted keys.
"""
from __future__ import annotations

import argparse
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from filler import fill_module, fill_value  # noqa: E402
from gen_inference_golden import write_npz  # noqa: E402

FILE_CAP = 900 * 1024   # bytes of raw array data per file (random floats do not compress)

# case -> B, nH, Hp, Wp, ws, shift (tests/test_swin_gpu.py has what each one reaches)
OP_CASES = {
    "a": (2, 2, 14, 21, 7, 0),
    "b": (2, 2, 14, 21, 7, 3),
    "c": (1, 3, 7, 7, 7, 3),
    "d": (2, 1, 24, 36, 12, 6),
    "e": (1, 2, 24, 12, 12, 0),
    "f": (1, 2, 10, 15, 5, 2),
}
TINY = dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0)
TINY_INPUT = (2, 3, 64, 96)
BLOCK = dict(dim=64, num_heads=2, window_size=7, shift_size=3, H=13, W=17, B=2)
FULL_GRAD = ("relative_position_bias_table", "qkv.bias")


def install_stubs():
    def have(name):
        try:
            return importlib.util.find_spec(name) is not None
        except (ImportError, ValueError):
            return False

    if not have("timm"):
        class DropPath(nn.Module):
            def __init__(self, p=0.0):
                super().__init__()
                assert p == 0.0, "the generator runs with drop_path_rate 0"

            def forward(self, x):
                return x

        layers = types.ModuleType("timm.models.layers")
        layers.DropPath = DropPath
        layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        layers.trunc_normal_ = nn.init.trunc_normal_
        for name in ("timm", "timm.models"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["timm.models.layers"] = layers
    if not have("detectron2"):
        class Registry:
            def register(self):
                return lambda cls: cls

        modeling = types.ModuleType("detectron2.modeling")
        modeling.BACKBONE_REGISTRY = Registry()
        modeling.Backbone = nn.Module
        modeling.ShapeSpec = lambda **kw: types.SimpleNamespace(**kw)
        sys.modules["detectron2"] = types.ModuleType("detectron2")
        sys.modules["detectron2.modeling"] = modeling


def import_reference_swin(ref_root):
    install_stubs()
    path = os.path.join(ref_root, "mask2former", "modeling", "backbone", "swin.py")
    spec = importlib.util.spec_from_file_location("reference_swin", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dist(a32, a64):
    a32, a64 = a32.detach().double(), a64.detach()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


class _Recorder(nn.Module):
    def forward(self, x, mask):
        self.mask = mask
        return x


class _Hand(nn.Module):
    """Stands where WindowAttention.qkv stood and hands over the qkv computed outside."""

    def __init__(self, windows):
        super().__init__()
        self.windows = windows

    def forward(self, x):
        return self.windows


def reference_core(ref, qkv, table, nH, ws, shift):
    """The reference's path from the qkv linear's output to the proj linear's input."""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    mask = None
    if shift > 0:
        layer = ref.BasicLayer(dim=C, depth=1, num_heads=nH, window_size=ws)
        assert layer.shift_size == shift
        rec = _Recorder()
        layer.blocks = nn.ModuleList([rec])
        layer(torch.zeros(1, Hp * Wp, C), Hp, Wp)
        mask = rec.mask
    attn = ref.WindowAttention(C, (ws, ws), nH).to(qkv.dtype)
    del attn.relative_position_bias_table
    attn.relative_position_bias_table = table          # a plain tensor: gradients flow to the caller's leaf
    attn.proj = nn.Identity()
    shifted = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    windows = ref.window_partition(shifted, ws).view(-1, ws * ws, C3)
    attn.qkv = _Hand(windows)
    o = attn(torch.zeros(windows.shape[0], ws * ws, C, dtype=qkv.dtype), mask=mask)
    o = ref.window_reverse(o.view(-1, ws, ws, C), ws, Hp, Wp)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else o


def gen_op_case(ref, name, case):
    B, nH, Hp, Wp, ws, shift = case
    C = nH * 32
    g = torch.Generator().manual_seed(1000 + ord(name))
    qkv = torch.randn(B, Hp, Wp, 3 * C, generator=g)
    gout = torch.randn(B, Hp, Wp, C, generator=g)
    table = fill_value(f"swin_op_{name}.relative_position_bias_table", ((2 * ws - 1) ** 2, nH)).float()
    res = {}
    for dt in (torch.float32, torch.float64):
        q = qkv.to(dt).clone().requires_grad_()
        t = table.to(dt).clone().requires_grad_()
        out = reference_core(ref, q, t, nH, ws, shift)
        out.backward(gout.to(dt))
        res[dt] = (out.detach(), q.grad, t.grad)
    o64, dq64, dt64 = res[torch.float64]
    o32, dq32, dt32 = res[torch.float32]
    return {"meta": np.array(case, dtype=np.int64), "qkv": qkv.numpy(), "gout": gout.numpy(), "table": table.numpy(),
            "out": o64.numpy(), "dqkv": dq64.numpy(), "dtable": dt64.numpy(),
            "floor": np.array([dist(o32, o64), dist(dq32, dq64), dist(dt32, dt64)])}


def gen_block(ref):
    c = BLOCK
    blk = ref.SwinTransformerBlock(dim=c["dim"], num_heads=c["num_heads"], window_size=c["window_size"],
                                   shift_size=c["shift_size"])
    fill_module(blk)
    layer = ref.BasicLayer(dim=c["dim"], depth=2, num_heads=c["num_heads"], window_size=c["window_size"])
    rec = _Recorder()
    layer.blocks = nn.ModuleList([rec])
    layer(torch.zeros(1, c["H"] * c["W"], c["dim"]), c["H"], c["W"])
    g = torch.Generator().manual_seed(77)
    x = torch.randn(c["B"], c["H"] * c["W"], c["dim"], generator=g)
    ys = {}
    for dt in (torch.float32, torch.float64):
        b = copy.deepcopy(blk).to(dt)
        b.H, b.W = c["H"], c["W"]
        ys[dt] = b(x.to(dt), rec.mask).detach()
    return {"meta": np.array([c["B"], c["H"], c["W"], c["dim"], c["num_heads"], c["window_size"], c["shift_size"]],
                             dtype=np.int64),
            "x": x.numpy(), "y": ys[torch.float64].numpy(), "floor": np.array([dist(ys[torch.float32], ys[torch.float64])])}


def gen_tiny(ref):
    model = ref.SwinTransformer(**TINY)
    fill_module(model)
    model.train()
    g = torch.Generator().manual_seed(2024)
    x = torch.randn(*TINY_INPUT, generator=g)
    runs = {}
    gs = None
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(model).to(dt)
        xi = x.to(dt).clone().requires_grad_()
        feats = m(xi)
        if gs is None:
            gs = {k: torch.randn(v.shape, generator=g) for k, v in feats.items()}
        loss = sum((feats[k] * gs[k].to(dt)).mean() for k in sorted(feats))
        loss.backward()
        runs[dt] = (feats, xi.grad, {k: p.grad for k, p in m.named_parameters()})
    f64, dx64, pg64 = runs[torch.float64]
    f32, dx32, pg32 = runs[torch.float32]
    res = {"x": x.numpy(), "dx": dx64.numpy(), "dx_floor": np.array([dist(dx32, dx64)])}
    for k in sorted(f64):
        res[k] = f64[k].detach().numpy()
        res[f"g_{k}"] = gs[k].numpy()
        res[f"{k}_floor"] = np.array([dist(f32[k], f64[k])])
    sums, sum_names = [], []
    for k in sorted(pg64):
        gr = pg64[k]
        parts = k.split(".")
        if k.endswith(FULL_GRAD) or (parts[-1] == "weight" and parts[-2].startswith("norm")):
            res[f"grad:{k}"] = gr.numpy()
            res[f"grad_floor:{k}"] = np.array([dist(pg32[k], gr)])
        else:
            sum_names.append(k)
            sums.append([float(gr.sum()), float(gr.abs().sum()), float(pg32[k].double().sum()),
                         float(pg32[k].double().abs().sum())])
    res["grad_sum_names"] = np.array(sum_names)
    res["grad_sums"] = np.array(sums)     # fp64 sum, fp64 abs sum, the reference's fp32 sum, fp32 abs sum
    sd = model.state_dict()
    res["state_keys"] = np.array(list(sd.keys()))
    shapes = np.full((len(sd), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    res["state_shapes"] = shapes
    return res


def write_split(out_dir, prefix, arrays):
    """Pack `arrays` into <prefix>_<n>.npz files of at most FILE_CAP bytes, splitting big arrays along axis 0."""
    items = []
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        if a.nbytes > FILE_CAP:
            n = -(-a.nbytes // FILE_CAP)
            assert a.shape[0] >= n, (k, a.shape)
            for i, part in enumerate(np.array_split(a, n, axis=0)):
                assert part.nbytes <= FILE_CAP, (k, part.shape)
                items.append((f"{k}__p{i}", part))
        else:
            items.append((k, a))
    files, cur, size = [], {}, 0
    for k, a in items:
        if cur and size + a.nbytes > FILE_CAP:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    files.append(cur)
    for i, f in enumerate(files):
        path = os.path.join(out_dir, f"{prefix}_{i}.npz")
        write_npz(path, f)
        assert os.path.getsize(path) < (1 << 20), path
    return len(files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(1)
    ref = import_reference_swin(a.ref)
    n = 0
    for name, case in OP_CASES.items():
        n += write_split(a.out, f"swin_op_{name}", gen_op_case(ref, name, case))
    n += write_split(a.out, "swin_block", gen_block(ref))
    n += write_split(a.out, "swin_tiny", gen_tiny(ref))
    print("wrote", n, "swin fixture files")


if __name__ == "__main__":
    main()
