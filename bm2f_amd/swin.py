"""Swin Transformer backbone on the fused shifted-window attention kernels (csrc/window_attn.hip).

Drop-in for the reference's ``mask2former/modeling/backbone/swin.py``: the same constructor arguments, the same
``cfg.MODEL.SWIN.*`` keys, the same state-dict keys and shapes (the ``relative_position_index`` buffers included, so a
reference checkpoint loads with ``strict=True``), the same outputs.  What differs is the inside of a block: the qkv
linear writes ``(B, Hp, Wp, 3C)`` and :func:`window_attention` turns it into ``(B, Hp, Wp, C)`` for the proj linear in
one kernel each way; the cyclic shift, the window partition, the relative-position-bias gather and the shift mask are
addresses inside the kernels, so no rolled, partitioned or reversed copy, no ``(nW*B, nH, N, N)`` score tensor and no
``(nW, N, N)`` mask exist.  qkv, proj, the MLP, LayerNorm, GELU, patch embed and patch merging stay in torch.

CUDA tensors go to ``libbm2f`` (a missing library or an unsupported shape raises: no fallback); CPU tensors run the
same definition in plain torch (roll, partition, matmul, analytic mask), differentiable by autograd.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .registry import BACKBONE_REGISTRY, Backbone, ShapeSpec, register

HEAD_DIM = 32   # every Swin variant; the only head dim the kernels are built for
MASKED = -100.0   # reference swin.py:438


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def relative_position_index(ws: int) -> torch.Tensor:
    """(N, N) int64: row of the ((2ws-1)^2, nH) bias table for query token i and key token j."""
    t = torch.arange(ws * ws)
    ty, tx = t // ws, t % ws
    return (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + (tx[:, None] - tx[None, :] + ws - 1)


def shift_regions(hp: int, wp: int, ws: int, shift: int, device=None) -> torch.Tensor:
    """(hp, wp) int64 nine-region labels of the shifted map (reference :416-431): along each axis 0 below
    ``n - ws``, 1 below ``n - shift``, else 2."""
    def axis(n):
        c = torch.arange(n, device=device)
        return (c >= n - ws).long() + (c >= n - shift).long()
    return 3 * axis(hp)[:, None] + axis(wp)[None, :]


def _partition(x, ws):
    """(B, Hp, Wp, ...) -> (B, nW, N, ...)"""
    B, Hp, Wp = x.shape[:3]
    rest = x.shape[3:]
    x = x.reshape(B, Hp // ws, ws, Wp // ws, ws, *rest)
    return x.permute(0, 1, 3, 2, 4, *range(5, x.dim())).reshape(B, (Hp // ws) * (Wp // ws), ws * ws, *rest)


def window_attention_torch(qkv, bias_table, num_heads, window_size, shift, scale=None, return_attn=False):
    """The definition in plain torch; softmax in fp32 whatever the dtype (as autocast runs it)."""
    B, Hp, Wp, C3 = qkv.shape
    ws, nH = window_size, num_heads
    D = C3 // (3 * nH)
    scale = D ** -0.5 if scale is None else scale
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    x = _partition(x, ws)                                              # (B, nW, N, 3C)
    nW, N = x.shape[1], x.shape[2]
    q, k, v = x.reshape(B, nW, N, 3, nH, D).permute(3, 0, 1, 4, 2, 5)    # each (B, nW, nH, N, D)
    attn = (q * scale) @ k.transpose(-2, -1)
    idx = relative_position_index(ws).to(qkv.device)
    bias = bias_table[idx.reshape(-1)].reshape(N, N, nH).permute(2, 0, 1)
    attn = attn + bias.to(attn.dtype)
    if shift > 0:
        lab = _partition(shift_regions(Hp, Wp, ws, shift, qkv.device)[None], ws)[0]    # (nW, N)
        mask = (lab[:, :, None] != lab[:, None, :]).to(attn.dtype) * MASKED
        attn = attn + mask[None, :, None]
    soft_dtype = torch.float32 if attn.dtype in (torch.float16, torch.bfloat16) else attn.dtype
    attn = torch.softmax(attn.to(soft_dtype), dim=-1)
    if return_attn:
        return attn
    out = attn.to(v.dtype) @ v                                          # (B, nW, nH, N, D)
    out = out.permute(0, 1, 3, 2, 4).reshape(B, Hp // ws, Wp // ws, ws, ws, nH * D)
    out = out.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, nH * D)
    return torch.roll(out, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else out


class _WindowAttention(Function):
    @staticmethod
    def forward(ctx, qkv, bias_table, num_heads, window_size, shift, scale):
        B, Hp, Wp, C3 = qkv.shape
        qkv = qkv.contiguous()
        table = bias_table.detach().to(torch.float32).contiguous()
        C = C3 // 3
        out = torch.empty(B, Hp, Wp, C, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, num_heads, Hp * Wp, device=qkv.device, dtype=torch.float32)
        with torch.cuda.device(qkv.device):   # the launch goes to the tensors' device, current or not
            _native.call("m2f_window_attn_fwd", _native.dtype_code(qkv.dtype, "window_attention"), qkv.data_ptr(),
                         table.data_ptr(), B, num_heads, C // num_heads, Hp, Wp, window_size, shift, scale,
                         out.data_ptr(), lse.data_ptr(), _native.stream(qkv))
        ctx.save_for_backward(qkv, table, lse)
        ctx.meta = (num_heads, window_size, shift, scale, bias_table.dtype)
        return out

    @staticmethod
    @once_differentiable   # the backward kernel is not itself differentiable: a double backward raises
    def backward(ctx, grad):
        qkv, table, lse = ctx.saved_tensors
        need_qkv, need_table = ctx.needs_input_grad[:2]
        if not (need_qkv or need_table):
            return None, None, None, None, None, None
        nH, ws, shift, scale, table_dtype = ctx.meta
        B, Hp, Wp, C3 = qkv.shape
        grad = grad.contiguous()
        dqkv = torch.empty_like(qkv)
        dtable = torch.empty_like(table)
        work = _native.workspace("m2f_window_attn_workspace", B, nH, Hp, Wp, ws, device=qkv.device, floor=16)
        # one kernel produces both gradients (the table's falls out of the dS it computes for dqkv anyway); a
        # gradient nobody asked for is dropped here
        with torch.cuda.device(qkv.device):
            _native.call("m2f_window_attn_bwd", _native.dtype_code(qkv.dtype, "window_attention"), qkv.data_ptr(),
                         table.data_ptr(), grad.data_ptr(), lse.data_ptr(), B, nH, C3 // (3 * nH), Hp, Wp, ws, shift,
                         scale, dqkv.data_ptr(), dtable.data_ptr(), work.data_ptr(), work.numel(), _native.stream(qkv))
        return (dqkv if need_qkv else None, dtable.to(table_dtype) if need_table else None, None, None, None, None)


def window_attention(qkv, bias_table, num_heads, window_size, shift, scale=None):
    """Shifted-window multi-head attention with relative-position bias.

    qkv ``(B, Hp, Wp, 3C)`` as ``nn.Linear(C, 3C)`` writes it (``[q | k | v]``, each ``num_heads x 32``), Hp and Wp
    multiples of ``window_size``; bias_table ``((2ws-1)^2, num_heads)``; ``shift`` in ``[0, window_size)``.  Returns
    ``(B, Hp, Wp, C)`` in the unshifted, unpartitioned layout.  Equal to the reference's roll -> window_partition ->
    WindowAttention core -> window_reverse -> roll (swin.py:131-171, :257-284)."""
    if qkv.dim() != 4 or qkv.shape[-1] % (3 * num_heads) != 0:
        raise ValueError(f"qkv must be (B, Hp, Wp, 3 * num_heads * head_dim), got {tuple(qkv.shape)}")
    ws = int(window_size)
    if qkv.shape[1] % ws or qkv.shape[2] % ws:
        raise ValueError(f"grid {qkv.shape[1]} x {qkv.shape[2]} is not a multiple of the window size {ws}")
    if not 0 <= shift < ws:
        raise ValueError(f"shift {shift} outside [0, {ws})")
    tw = (2 * ws - 1) ** 2
    if tuple(bias_table.shape) != (tw, num_heads):
        raise ValueError(f"bias_table must be ({tw}, {num_heads}), got {tuple(bias_table.shape)}")
    head_dim = qkv.shape[-1] // (3 * num_heads)
    scale = float(head_dim ** -0.5 if scale is None else scale)
    if not qkv.is_cuda:
        return window_attention_torch(qkv, bias_table, num_heads, ws, int(shift), scale)
    if qkv.dtype not in _native.DTYPE_CODES:
        raise TypeError(f"window_attention on the device takes fp32, fp16 or bf16, got {qkv.dtype}")
    # an unsupported window size or head dim is refused by the library (NativeError): there is no other device path
    return _WindowAttention.apply(qkv, bias_table, num_heads, ws, int(shift), scale)


class DropPath(nn.Module):
    """Per-sample stochastic depth on the residual branch (Huang et al. 2016), kept branches rescaled by 1/keep."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        if keep > 0.0:
            mask = mask / keep
        return x * mask

    def extra_repr(self):
        return f"drop_prob={self.drop_prob:.3f}"


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class WindowAttention(nn.Module):
    """W-MSA / SW-MSA with relative position bias over a whole (padded) feature map.

    ``forward(x, shift)`` takes ``(B, Hp, Wp, C)`` and returns the same shape: the reference's partitioned
    ``(nW*B, N, C)`` input and ``(nW, N, N)`` mask do not exist here."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        if attn_drop != 0.0:
            raise NotImplementedError("attention dropout inside the fused softmax is not built (every shipped config "
                                      "uses ATTN_DROP_RATE 0.0)")
        self.dim = dim
        self.window_size = _pair(window_size)
        if self.window_size[0] != self.window_size[1]:
            raise NotImplementedError("square windows only")
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        ws = self.window_size[0]
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        # kept for state-dict parity with the reference; the kernels compute the index from token coordinates
        self.register_buffer("relative_position_index", relative_position_index(ws))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x, shift=0):
        x = window_attention(self.qkv(x), self.relative_position_bias_table, self.num_heads, self.window_size[0],
                             shift, self.scale)
        return self.proj_drop(self.proj(x))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=_pair(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.H = None
        self.W = None

    def forward(self, x, mask_matrix=None):
        """x (B, H*W, C) with ``self.H``, ``self.W`` set by the layer; ``mask_matrix`` is accepted for the reference's
        calling convention and unused (the kernels compute the shift mask)."""
        B, L, C = x.shape
        H, W = self.H, self.W
        assert L == H * W, "input feature has wrong size"
        ws = self.window_size
        shortcut = x
        x = self.norm1(x).view(B, H, W, C)
        # pad after norm1, before qkv, as the reference: padded tokens carry the qkv bias and are unmasked keys
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        if pad_r or pad_b:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        x = self.attn(x, self.shift_size)
        if pad_r or pad_b:
            x = x[:, :H, :W, :].contiguous()
        x = shortcut + self.drop_path(x.view(B, H * W, C))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        x = x.view(B, H, W, C)
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if i % 2 == 0 else window_size // 2, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x, H, W):
        for blk in self.blocks:
            blk.H, blk.W = H, W
            if self.use_checkpoint:
                x = checkpoint.checkpoint(blk, x, use_reentrant=False)
            else:
                x = blk(x)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = _pair(patch_size)
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        H, W = x.shape[-2:]
        ph, pw = self.patch_size
        if W % pw != 0:
            x = F.pad(x, (0, pw - W % pw))
        if H % ph != 0:
            x = F.pad(x, (0, 0, 0, ph - H % ph))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.shape[2], x.shape[3]
            x = self.norm(x.flatten(2).transpose(1, 2))
            x = x.transpose(1, 2).view(-1, self.embed_dim, Wh, Ww)
        return x


class SwinTransformer(nn.Module):
    """Swin Transformer backbone (Liu et al. 2021) returning ``{"res2": ..., "res5": ...}`` NCHW feature maps."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.2, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 out_indices=(0, 1, 2, 3), frozen_stages=-1, use_checkpoint=False):
        super().__init__()
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.out_indices = out_indices
        self.frozen_stages = frozen_stages
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if self.patch_norm else None)
        if self.ape:
            size, patch = _pair(pretrain_img_size), _pair(patch_size)
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, size[0] // patch[0], size[1] // patch[1]))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=0.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(BasicLayer(
                dim=int(embed_dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size,
                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if i < self.num_layers - 1 else None, use_checkpoint=use_checkpoint))
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i in out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 1 and self.ape:
            self.absolute_pos_embed.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                m = self.layers[i]
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def forward(self, x):
        x = self.patch_embed(x)
        Wh, Ww = x.size(2), x.size(3)
        if self.ape:
            pos = F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode="bicubic")
            x = (x + pos).flatten(2).transpose(1, 2)
        else:
            x = x.flatten(2).transpose(1, 2)
        x = self.pos_drop(x)
        outs = {}
        for i in range(self.num_layers):
            x_out, H, W, x, Wh, Ww = self.layers[i](x, Wh, Ww)
            if i in self.out_indices:
                x_out = getattr(self, f"norm{i}")(x_out)
                outs[f"res{i + 2}"] = x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous()
        return outs

    def train(self, mode=True):
        """Training mode with the frozen stages kept in eval."""
        super().train(mode)
        self._freeze_stages()
        return self


@register(lambda: BACKBONE_REGISTRY)
class D2SwinTransformer(SwinTransformer, Backbone):
    def __init__(self, cfg, input_shape=None):
        s = cfg.MODEL.SWIN
        super().__init__(s.PRETRAIN_IMG_SIZE, s.PATCH_SIZE, 3, s.EMBED_DIM, s.DEPTHS, s.NUM_HEADS, s.WINDOW_SIZE,
                         s.MLP_RATIO, s.QKV_BIAS, s.QK_SCALE, s.DROP_RATE, s.ATTN_DROP_RATE, s.DROP_PATH_RATE,
                         nn.LayerNorm, s.APE, s.PATCH_NORM, use_checkpoint=s.USE_CHECKPOINT)
        self._out_features = s.OUT_FEATURES
        self._out_feature_strides = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}
        self._out_feature_channels = {f"res{i + 2}": self.num_features[i] for i in range(4)}

    def forward(self, x):
        assert x.dim() == 4, f"SwinTransformer takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        y = super().forward(x)
        return {k: v for k, v in y.items() if k in self._out_features}

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    @property
    def size_divisibility(self):
        return 32


__all__ = ["window_attention", "window_attention_torch", "relative_position_index", "shift_regions", "DropPath", "Mlp",
           "WindowAttention", "SwinTransformerBlock", "PatchMerging", "BasicLayer", "PatchEmbed", "SwinTransformer",
           "D2SwinTransformer"]
