"""Box-supervised (weak-supervision) ops on the gfx950 kernels of ``csrc/weaksup.hip`` and ``csrc/lsap.hip``:
batched Hungarian matching, the pairwise-affinity cost / loss, neighbour-similarity bits and the GPU target
preparation that replaces the reference's per-image host loop with skimage.

The pairwise, LSAP and target-preparation ops here take CUDA tensors and raise on anything else: they have no CPU
path (the CPU restatement lives in ``oracle/weaksup_ref.py`` and is test infrastructure only), so the image
criterion's losses need HIP tensors.  Its matcher is the video matcher on one-frame clips and, like that one, evaluates
its definition in plain torch (scipy for the assignment) on CPU tensors without calling these ops.  The temporal-pair
ops of the video criterion (``csrc/video_pairs.hip``: packing, the temporal pairwise sum, pair mining) also evaluate
their definition in plain torch on CPU tensors, like ``inference.py``.
"""
from __future__ import annotations

from typing import List, Sequence

import torch
from torch.autograd import Function

from . import _native


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("bm2f_amd.weaksup ops need CUDA (HIP) tensors; there is no CPU path")


def h2d(values: Sequence[int], device, dtype=torch.int32) -> torch.Tensor:
    """Small host list -> device tensor without a stream synchronisation (pinned, non-blocking)."""
    t = torch.tensor(list(values), dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True)


# --------------------------------------------------------------------------------------------------------
# linear sum assignment
# --------------------------------------------------------------------------------------------------------
LSAP_STATUS = {1: "cost matrix is infeasible", 2: "problem too large for the GPU solver",
               3: "matrix contains invalid numeric entries"}


def lsap_batched(cost: torch.Tensor, cols: torch.Tensor | None = None, rows: torch.Tensor | None = None):
    """Solve ``cost[b, :rows[b], :cols[b]]`` for every b (scipy.optimize.linear_sum_assignment semantics).

    cost (B, R, C) fp32 (made contiguous); rows / cols int32 device tensors (default: full).  Returns
    ``match`` (B, R) int32 (column matched to row r, -1 if none) and ``status`` (B,) int32 (0 = ok, see
    LSAP_STATUS).  No host synchronisation.
    """
    _need_cuda(cost)
    if cost.dim() != 3:
        raise ValueError("cost must be (B, R, C)")
    B, R, C = cost.shape
    c = cost.float().contiguous()
    dev = c.device
    if rows is None:
        rows = torch.full((B,), R, dtype=torch.int32, device=dev)
    match = torch.empty((B, R), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if B == 0 or R == 0:
        return match, status
    _native.call("m2f_lsap_batched", c.data_ptr(), B, R, C, R * C, rows.data_ptr(), _native.ptr(cols),
                 match.data_ptr(), status.data_ptr(), _native.stream(c))
    return match, status


def raise_on_lsap_status(status: torch.Tensor) -> None:
    """Raise ValueError like scipy for a failed problem (one host sync)."""
    s = status.max().item() if status.numel() else 0
    if s:
        raise ValueError(LSAP_STATUS.get(int(s), f"linear_sum_assignment failed ({s})"))


def indices_from_match(match: torch.Tensor, n_matched: Sequence[int]) -> List[tuple]:
    """(B, Q) match rows -> per image (query idx, target idx) int64, queries ascending (scipy's order).

    ``n_matched[b]`` (= min(Q, G_b), known on the host) sizes each slice, so nothing syncs.  Works on any
    device."""
    B, Q = match.shape
    if B == 0:
        return []
    ar = torch.arange(Q, device=match.device, dtype=torch.int64)
    key = torch.where(match >= 0, ar[None], torch.full_like(ar, Q)[None])
    src = key.sort(dim=1).values
    tgt = match.long().gather(1, src.clamp(max=Q - 1))
    return [(src[b, :n], tgt[b, :n]) for b, n in enumerate(n_matched)]


# --------------------------------------------------------------------------------------------------------
# pairwise affinity
# --------------------------------------------------------------------------------------------------------
def threshold_bits(sim: torch.Tensor, thr: float) -> torch.Tensor:
    """(N, 8, H, W) similarity -> (N, H, W) uint8 neighbour bits, bit k = sim[:, k] >= thr."""
    _need_cuda(sim)
    if sim.dim() != 4 or sim.shape[1] != 8:
        raise ValueError("similarity must be (N, 8, H, W) (pairwise_size 3)")
    s = sim.float().contiguous()
    N, _, H, W = s.shape
    bits = torch.empty((N, H, W), dtype=torch.uint8, device=s.device)
    _native.call("m2f_threshold_bits", s.data_ptr(), N, H * W, thr, bits.data_ptr(), _native.stream(s))
    return bits


def _rows_args(x, bits, t_row, box, box_row, dilation):
    _need_cuda(x, bits, t_row, box, box_row)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 3:
        raise ValueError("x must be a contiguous fp32 (N, H, W) tensor")
    for t in (t_row, box_row):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError("row index tensors must be contiguous int32")
    if box is not None and (box.dtype != torch.float32 or not box.is_contiguous()):
        raise ValueError("box must be contiguous fp32")
    if bits is not None and (bits.dtype != torch.uint8 or not bits.is_contiguous()):
        raise ValueError("bits must be contiguous uint8")
    if dilation < 1 or dilation > 4:
        raise ValueError("pairwise_dilation must be in [1, 4]")


def pairwise_map(x: torch.Tensor, bits: torch.Tensor, t_row: torch.Tensor, dilation: int) -> torch.Tensor:
    """out[r, p] = sum_k bit_k s_k(p) over rows of x (N, H, W); row r uses bits[t_row[r]]."""
    _rows_args(x, bits, t_row, None, None, dilation)
    N, H, W = x.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    _native.call("m2f_pairwise_rows", x.data_ptr(), None, N, H, W, dilation, bits.data_ptr(), t_row.data_ptr(), None,
                 None, 0, out.data_ptr(), None, _native.stream(x))
    return out


def pairwise_planes(x: torch.Tensor, dilation: int) -> torch.Tensor:
    """(N, H, W) logits -> (N, 8, H, W) s_k(p) = -log P(p and its k-th neighbour share a label)."""
    _rows_args(x, None, None, None, None, dilation)
    N, H, W = x.shape
    out = torch.empty((N, 8, H, W), dtype=torch.float32, device=x.device)
    _native.call("m2f_pairwise_rows", x.data_ptr(), None, N, H, W, dilation, None, None, None, None, 2, out.data_ptr(),
                 None, _native.stream(x))
    return out


def box_extents(box: torch.Tensor) -> torch.Tensor:
    """(B, G, H, W) masks -> (B, G, 4) int32 [y0, y1, x0, x1) bounding every nonzero pixel (empty: y0 = H)."""
    B, G, H, W = box.shape
    rows = box.ne(0).any(3)                                    # (B, G, H)
    cols = box.ne(0).any(2)                                    # (B, G, W)
    ar_h = torch.arange(H, device=box.device)
    ar_w = torch.arange(W, device=box.device)
    y0 = torch.where(rows, ar_h, H).amin(2)
    y1 = torch.where(rows, ar_h + 1, 0).amax(2)
    x0 = torch.where(cols, ar_w, W).amin(2)
    x1 = torch.where(cols, ar_w + 1, 0).amax(2)
    return torch.stack([y0, y1, x0, x1], -1).to(torch.int32).contiguous()


def match_cost(x: torch.Tensor, bits: torch.Tensor, box: torch.Tensor, gcount: torch.Tensor, dilation: int,
               extents: torch.Tensor | None = None):
    """The matcher's fused pass (``m2f_pairwise_match_cost``) over mask logits x (B, Q, H, W):

    returns num (B, Q, Gm) = sum_p box[b, g, p] sum_k bit_k(p) s_k(p) (0 for g >= gcount[b]), and the axis
    projections x.amax(3) (B, Q, H), x.amax(2) (B, Q, W) -- one read of x instead of three.  ``extents``
    (from :func:`box_extents`) lets the kernel skip tiles a target's mask does not touch."""
    _need_cuda(x, bits, box, gcount)
    if extents is None:
        extents = box_extents(box)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4:
        raise ValueError("x must be a contiguous fp32 (B, Q, H, W) tensor")
    if box.dtype != torch.float32 or not box.is_contiguous() or gcount.dtype != torch.int32:
        raise ValueError("box must be contiguous fp32 (B, Gm, H, W), gcount int32")
    B, Q, H, W = x.shape
    Gm = box.shape[1]
    lib = _native.load()
    tiles = lib.m2f_pairwise_tiles(H, W)
    ntx, nty = (W + 63) // 64, (H + 15) // 16
    part = torch.empty((B * Q, tiles, Gm), dtype=torch.float32, device=x.device)
    rmax = torch.empty((B * Q, H, ntx), dtype=torch.float32, device=x.device)
    cmax = torch.empty((B * Q, nty, W), dtype=torch.float32, device=x.device)
    _native.call("m2f_pairwise_match_cost", x.data_ptr(), B, Q, H, W, dilation, bits.data_ptr(), box.data_ptr(),
                 gcount.data_ptr(), extents.data_ptr(), Gm, part.data_ptr(), rmax.data_ptr(), cmax.data_ptr(),
                 _native.stream(x))
    return (part.sum(1).view(B, Q, Gm), rmax.amax(2).view(B, Q, H), cmax.amax(1).view(B, Q, W))


class PairwiseSums(Function):
    """Per-row ``num[r] = sum_{p,k} box(p) bit_k(p) s_k(p)`` and ``den[r] = sum_{p,k} box(p) bit_k(p)``;
    differentiable in the mask logits x (criterion.py:156-181 + 300-311, fused)."""

    @staticmethod
    def forward(ctx, x, bits, t_row, box, box_row, dilation):
        _rows_args(x, bits, t_row, box, box_row, dilation)
        N, H, W = x.shape
        lib = _native.load()
        tiles = lib.m2f_pairwise_tiles(H, W)
        num = torch.empty((N, max(tiles, 1)), dtype=torch.float32, device=x.device)
        den = torch.empty_like(num)
        if N and H and W:
            _native.call("m2f_pairwise_rows", x.data_ptr(), None, N, H, W, dilation, bits.data_ptr(),
                         _native.ptr(t_row), _native.ptr(box), _native.ptr(box_row), 1, num.data_ptr(), den.data_ptr(),
                         _native.stream(x))
        else:
            num.zero_()
            den.zero_()
        ctx.save_for_backward(x, bits, t_row, box, box_row)
        ctx.dilation = dilation
        num_r, den_r = num.sum(1), den.sum(1)
        ctx.mark_non_differentiable(den_r)
        return num_r, den_r

    @staticmethod
    def backward(ctx, g_num, g_den):
        x, bits, t_row, box, box_row = ctx.saved_tensors
        N, H, W = x.shape
        grad = torch.empty_like(x)
        if N and H and W:
            g = g_num.float().contiguous()
            _native.call("m2f_pairwise_rows_bwd", x.data_ptr(), None, N, H, W, ctx.dilation, bits.data_ptr(),
                         _native.ptr(t_row), _native.ptr(box), _native.ptr(box_row), g.data_ptr(), grad.data_ptr(),
                         _native.stream(x))
        return grad, None, None, None, None, None


def pairwise_sums(x, bits, t_row, box, box_row, dilation):
    return PairwiseSums.apply(x, bits, t_row, box, box_row, dilation)


# --------------------------------------------------------------------------------------------------------
# temporal pairs of the video criterion (mask2former_video/utils/weaksup_utils.py:64-165,
# modeling/criterion_proj_spatpair_temppair.py:25-69, :269-334).  Unlike the ops above these also accept CPU
# tensors and then evaluate the same definition in plain torch, so the video criterion's host logic is
# testable without a GPU; on a HIP tensor a kernel error raises, there is no fall-back.
# --------------------------------------------------------------------------------------------------------
class MinedPairs:
    """The temporal pairs of one clip in packed form: ``g`` (target), ``t`` (frame), ``p0`` / ``p1`` (linear
    pixel y*w + x in frame t / t+1), all (P,) int32 on the features' device and ordered by (g, t, current
    pixel row-major); ``counts`` (G, T-1) host ints = pairs per (target, frame pair)."""

    def __init__(self, g, t, p0, p1, counts, T, h, w):
        self.g, self.t, self.p0, self.p1 = g, t, p0, p1
        self.counts = counts
        self.T, self.h, self.w = int(T), int(h), int(w)

    def __len__(self):
        return len(self.counts)

    def to_lists(self):
        """The reference's nested ``[[(curr (k, 2), next (k, 2))] * (T-1)] * G`` int32 XY lists
        (video_maskformer_model.py:523-558); no host synchronisation."""
        w = self.w
        curr = torch.stack([self.p0 % w, self.p0 // w], 1)
        nxt = torch.stack([self.p1 % w, self.p1 // w], 1)
        sizes = [int(c) for row in self.counts for c in row]
        cs, ns = curr.split(sizes), nxt.split(sizes)
        n = self.T - 1
        return [[(cs[g * n + t], ns[g * n + t]) for t in range(n)] for g in range(len(self.counts))]


def _from_host(a, device):
    t = torch.from_numpy(a)
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else t


def _argmin_sqdist(a, b):
    """First arg-min over rows of b of sum_d (a - b)^2, rows of a in chunks (no full distance matrix)."""
    step = max(1, (1 << 22) // max(1, b.shape[0] * a.shape[1]))
    out = [((a[i:i + step, None] - b[None]) ** 2).sum(-1).argmin(1) for i in range(0, a.shape[0], step)]
    return torch.cat(out)


def temporal_pairs(feats: torch.Tensor, boxes: torch.Tensor, k: int = 1) -> MinedPairs:
    """Temporal pair mining for all instances and frame pairs of one clip (``get_instance_temporal_pairs``
    looped as in video_maskformer_model.py:523-558).

    feats (T, D, h, w) fp32; boxes (G, T, 4) integer XYXY, sliced half-open (``[y0:y1, x0:x1]``, clipped to
    the frame as slicing does).  For every instance and every t where both boxes have positive area, each
    pixel of the frame-t box (row-major) is paired with the frame-(t+1) box pixel at the smallest L2 feature
    distance; k == 1 on a HIP tensor is one launch of ``m2f_temporal_mine`` over all segments (distances as
    sums of (a-b)^2 in fp32, first minimum).  k > 1 is the reference's cdist().half().topk(k) in torch.
    The boxes are read on the host once."""
    if feats.dim() != 4 or boxes.dim() != 3 or boxes.shape[-1] != 4 or boxes.shape[1] != feats.shape[0]:
        raise ValueError("feats must be (T, D, h, w) and boxes (G, T, 4)")
    if boxes.is_floating_point() or k < 1:
        raise ValueError("boxes must be integer XYXY and k >= 1")
    import numpy as np
    T, D, h, w = feats.shape
    dev = feats.device
    bx = boxes.detach().cpu().numpy().astype(np.int64)
    if (bx < 0).any():
        raise ValueError("boxes must be non-negative pixel coordinates")
    G = bx.shape[0]
    bx = np.minimum(bx, np.array([w, h, w, h]))
    pos = (bx[..., 2] > bx[..., 0]) & (bx[..., 3] > bx[..., 1])
    counts = np.zeros((G, max(T - 1, 0)), np.int64)
    segs, blocks, g_l, t_l, p0_l = [], [], [], [], []
    off = 0
    for g in range(G):
        for t in range(T - 1):
            if not (pos[g, t] and pos[g, t + 1]):
                continue
            cx0, cy0, cx1, cy1 = bx[g, t]
            nx0, ny0, nx1, ny1 = bx[g, t + 1]
            cw, nw = cx1 - cx0, nx1 - nx0
            nc, nn = cw * (cy1 - cy0), nw * (ny1 - ny0)
            kk = min(k, nn)
            j = np.arange(nc)
            blocks += [(len(segs), c) for c in range((nc + 63) // 64)]
            segs.append((t, cx0, cy0, cw, nc, nx0, ny0, nw, nn, off))
            p0_l.append(np.repeat((cy0 + j // cw) * w + cx0 + j % cw, kk))
            g_l.append(np.full(nc * kk, g))
            t_l.append(np.full(nc * kk, t))
            counts[g, t] = nc * kk
            off += nc * kk
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)  # noqa: E731
    g_d, t_d, p0_d = (_from_host(cat(x), dev) for x in (g_l, t_l, p0_l))
    x = feats.float().contiguous()
    if k == 1 and x.is_cuda:
        p1 = torch.zeros(off, dtype=torch.int32, device=dev)
        if segs:
            seg_d = _from_host(np.asarray(segs, np.int32), dev)
            blk_d = _from_host(np.asarray(blocks, np.int32), dev)
            _native.call("m2f_temporal_mine", x.data_ptr(), T, D, h, w, seg_d.data_ptr(), len(segs), blk_d.data_ptr(),
                         len(blocks), p1.data_ptr(), off, _native.stream(x))
    else:
        parts = []
        for (t, cx0, cy0, cw, nc, nx0, ny0, nw, nn, _) in segs:
            a = x[t, :, cy0:cy0 + nc // cw, cx0:cx0 + cw].flatten(1).t()
            b = x[t + 1, :, ny0:ny0 + nn // nw, nx0:nx0 + nw].flatten(1).t()
            if k == 1:
                j = _argmin_sqdist(a, b)
            else:
                j = (-torch.cdist(a, b, p=2).half()).topk(k=min(k, nn), dim=1)[1].flatten()
            parts.append(((ny0 + j // nw) * w + nx0 + j % nw).to(torch.int32))
        p1 = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int32, device=dev)
    return MinedPairs(g_d, t_d, p0_d, p1, counts.tolist(), T, h, w)


class PackedPairs:
    """All temporal pairs of a batch of clips, packed once per criterion call: ``row`` (flat target row over
    the batch, -1 for a pair with an out-of-frame coordinate), ``t``, ``p0``, ``p1`` (P,) int32, and the
    2P endpoints sorted stably by ``ep_key`` = (row * T + frame) * H*W + pixel with ``ep_code`` = 2 * pair
    + side.  Runs of equal keys are the segments the backward kernel owns one thread each.  ``bad`` is a
    device bool: some pair was out of frame (checked with the matcher status, one sync per call)."""

    def __init__(self, row, t, p0, p1, ep_key, ep_code, n_targets, T, H, W, bad):
        self.row, self.t, self.p0, self.p1 = row, t, p0, p1
        self.ep_key, self.ep_code = ep_key, ep_code
        self.P = int(row.shape[0])
        self.n_targets, self.T, self.H, self.W = int(n_targets), int(T), int(H), int(W)
        self.bad = bad


def pack_temporal_pairs(per_clip, T: int, H: int, W: int, device) -> PackedPairs:
    """per_clip[b]: a :class:`MinedPairs` or the reference's nested lists (XY coordinates) of clip b's
    targets.  Sizes come from tensor shapes, so nothing synchronises."""
    import numpy as np
    rows, ts, c0, c1 = [], [], [], []
    off = 0
    for clip in per_clip:
        if isinstance(clip, MinedPairs):
            if (clip.T, clip.h, clip.w) != (T, H, W):
                raise ValueError("temporal pairs were mined at another clip size")
            if clip.g.numel():
                rows.append(clip.g.to(device).long() + off)
                ts.append(clip.t.to(device).long())
                c0.append(clip.p0.to(device).long())
                c1.append(clip.p1.to(device).long())
        else:
            r_h, t_h = [], []
            for g, per_frame in enumerate(clip):
                if len(per_frame) != T - 1:
                    raise ValueError("temporal_pairs needs T - 1 entries per target")
                for t, (cur, nxt) in enumerate(per_frame):
                    if cur.shape != nxt.shape:
                        raise ValueError("current / next pair coordinates differ in shape")
                    if cur.shape[0] == 0:
                        continue
                    r_h.append(np.full(cur.shape[0], off + g))
                    t_h.append(np.full(cur.shape[0], t))
                    cur, nxt = cur.to(device).long(), nxt.to(device).long()
                    ok = (cur[:, 0] >= 0) & (cur[:, 0] < W) & (cur[:, 1] >= 0) & (cur[:, 1] < H) & \
                         (nxt[:, 0] >= 0) & (nxt[:, 0] < W) & (nxt[:, 1] >= 0) & (nxt[:, 1] < H)
                    c0.append(torch.where(ok, cur[:, 1] * W + cur[:, 0], -1))
                    c1.append(torch.where(ok, nxt[:, 1] * W + nxt[:, 0], -1))
            if r_h:
                rows.append(_from_host(np.concatenate(r_h), device))
                ts.append(_from_host(np.concatenate(t_h), device))
        off += len(clip)
    if not rows:
        e32 = torch.zeros(0, dtype=torch.int32, device=device)
        return PackedPairs(e32, e32, e32, e32, torch.zeros(0, dtype=torch.int64, device=device), e32, off, T, H, W,
                           torch.zeros((), dtype=torch.bool, device=device))
    row, t, p0, p1 = (torch.cat(x) for x in (rows, ts, c0, c1))
    HW = H * W
    ok = (p0 >= 0) & (p0 < HW) & (p1 >= 0) & (p1 < HW) & (t >= 0) & (t < T - 1)
    row = torch.where(ok, row, -1)
    t, p0, p1 = (torch.where(ok, v, 0) for v in (t, p0, p1))
    keys = torch.stack([torch.where(ok, (row * T + t) * HW + p0, -1),
                        torch.where(ok, (row * T + t + 1) * HW + p1, -1)], 1).view(-1)
    ep_key, order = torch.sort(keys, stable=True)
    i32 = lambda v: v.to(torch.int32).contiguous()  # noqa: E731
    return PackedPairs(i32(row), i32(t), i32(p0), i32(p1), ep_key.contiguous(), i32(order), off, T, H, W,
                       (~ok).any())


def _pair_term_torch(a, b):
    """calculate_temp_similarities (criterion_proj_spatpair_temppair.py:56-69), the reference's own form."""
    import torch.nn.functional as F
    fg = F.logsigmoid(a) + F.logsigmoid(b)
    bg = F.logsigmoid(-a) + F.logsigmoid(-b)
    m = torch.max(fg, bg)
    return -(torch.log(torch.exp(fg - m) + torch.exp(bg - m)) + m)


class TemporalPairSum(Function):
    """(sum of s over the live pairs, their count) for matched masks src (N, T, H, W); differentiable in
    src.  The backward pass writes each touched pixel once, in a fixed order (bitwise repeatable)."""

    @staticmethod
    def forward(ctx, src, row_of_target, pk):
        N, T, H, W = src.shape
        nb = _native.load().m2f_temporal_blocks(pk.P)
        part_sum = torch.empty(nb, dtype=torch.float32, device=src.device)
        part_cnt = torch.empty(nb, dtype=torch.int32, device=src.device)
        _native.call("m2f_temporal_pairs_fwd", src.data_ptr(), N, T, H, W, row_of_target.data_ptr(), pk.n_targets,
                     pk.row.data_ptr(), pk.t.data_ptr(), pk.p0.data_ptr(), pk.p1.data_ptr(), pk.P,
                     part_sum.data_ptr(), part_cnt.data_ptr(), _native.stream(src))
        ctx.save_for_backward(src, row_of_target)
        ctx.pk = pk
        total, count = part_sum.sum(), part_cnt.sum()
        ctx.mark_non_differentiable(count)
        return total, count

    @staticmethod
    def backward(ctx, g_total, g_count):
        src, row_of_target = ctx.saved_tensors
        pk = ctx.pk
        N, T, H, W = src.shape
        grad = torch.zeros_like(src)
        g = g_total.float().reshape(1).contiguous()
        _native.call("m2f_temporal_pairs_bwd", src.data_ptr(), N, T, H, W, row_of_target.data_ptr(), pk.n_targets,
                     pk.row.data_ptr(), pk.t.data_ptr(), pk.p0.data_ptr(), pk.p1.data_ptr(), pk.P,
                     pk.ep_key.data_ptr(), pk.ep_code.data_ptr(), g.data_ptr(), grad.data_ptr(), _native.stream(src))
        return grad, None, None


def temporal_pair_sum(src: torch.Tensor, row_of_target: torch.Tensor, pk: PackedPairs):
    """Sum of the temporal pair terms of matched masks src (N, T, H, W) fp32 and the number of live pairs
    (an int tensor on src's device; no host synchronisation).  ``row_of_target`` (pk.n_targets,) int32 maps
    a flat target row to its row of src or -1; pairs of unmatched targets are dead."""
    if src.dim() != 4 or src.dtype != torch.float32 or (src.shape[1:] != (pk.T, pk.H, pk.W) and pk.P):
        raise ValueError("src must be fp32 (N, T, H, W) of the packed pairs' clip size")
    if row_of_target.dtype != torch.int32 or row_of_target.numel() != pk.n_targets:
        raise ValueError("row_of_target must be int32 with one entry per target")
    if src.is_cuda:
        _need_cuda(row_of_target, pk.row, pk.ep_key)
        return TemporalPairSum.apply(src.contiguous(), row_of_target.contiguous(), pk)
    N = src.shape[0]
    if N == 0 or pk.P == 0:
        return src.sum() * 0.0, torch.zeros((), dtype=torch.int64)
    HW = pk.H * pk.W
    n = torch.where(pk.row >= 0, row_of_target.long()[pk.row.clamp(min=0).long()], -1)
    live = n >= 0
    n = n[live]
    t, p0, p1 = pk.t.long()[live], pk.p0.long()[live], pk.p1.long()[live]
    flat = src.reshape(N, -1)
    s = _pair_term_torch(flat[n, t * HW + p0], flat[n, (t + 1) * HW + p1])
    return s.sum(), live.sum()


# --------------------------------------------------------------------------------------------------------
# target preparation (maskformer_model.py:399-507)
# --------------------------------------------------------------------------------------------------------
def images_lab(images: torch.Tensor, stride: int) -> torch.Tensor:
    """(B, 3, Hp, Wp) 0..255 padded images -> (B, 3, Hp/stride, Wp/stride) Lab (avg-pool, .byte(), rgb2lab)."""
    _need_cuda(images)
    x = images.float().contiguous()
    B, C, Hp, Wp = x.shape
    if C != 3:
        raise ValueError("images must have 3 channels")
    lab = torch.empty((B, 3, Hp // stride, Wp // stride), dtype=torch.float32, device=x.device)
    _native.call("m2f_weaksup_lab", x.data_ptr(), B, Hp, Wp, stride, lab.data_ptr(), _native.stream(x))
    return lab


def color_similarity(lab: torch.Tensor, mask: torch.Tensor, dilation: int) -> torch.Tensor:
    """lab (B, 3, h, w), mask (B, h, w) -> (B, 8, h, w) neighbour colour similarity."""
    _need_cuda(lab, mask)
    lab = lab.float().contiguous()
    mask = mask.float().contiguous()
    B, _, h, w = lab.shape
    sim = torch.empty((B, 8, h, w), dtype=torch.float32, device=lab.device)
    _native.call("m2f_color_similarity", lab.data_ptr(), mask.data_ptr(), B, h, w, dilation, sim.data_ptr(),
                 _native.stream(lab))
    return sim


def _pad_stack(tensors, size_divisibility, pad_value):
    """detectron2 ImageList.from_tensors: pad bottom/right to the max size rounded up, then stack."""
    hs = max(t.shape[-2] for t in tensors)
    ws = max(t.shape[-1] for t in tensors)
    if size_divisibility > 1:
        s = size_divisibility
        hs, ws = (hs + s - 1) // s * s, (ws + s - 1) // s * s
    out = tensors[0].new_full((len(tensors),) + tuple(tensors[0].shape[:-2]) + (hs, ws), pad_value)
    for i, t in enumerate(tensors):
        out[i, ..., :t.shape[-2], :t.shape[-1]].copy_(t)
    return out


def _boxes_and_labels(t):
    if isinstance(t, dict):
        return t["boxes"], t["labels"]
    return t.gt_boxes.tensor, t.gt_classes        # detectron2 Instances


def prepare_weaksup_targets(targets, org_images, img_heights, *, size_divisibility=32, mask_out_stride=4,
                            bottom_pixels_removed=10, pairwise_size=3, pairwise_dilation=2):
    """GPU ``MaskFormer.prepare_weaksup_targets`` (maskformer_model.py:399-507).

    targets: per image a detectron2 ``Instances`` (``gt_boxes.tensor`` (G, 4) x0,y0,x1,y1 and
    ``gt_classes``) or a dict with "boxes" / "labels"; org_images: per image (3, H, W) 0..255 (uint8 or
    float) CUDA tensors; img_heights: the annotation heights (bottom-pixel removal scales with them).

    Returns the reference's per-image dicts: labels, box_masks (G, h, w), images_color_similarity
    (G, 8, h, w) -- a zero-copy ``expand`` of the image's one similarity map (the reference materialises
    G identical copies), and the four projection bounds.  Differences: an image without boxes yields
    empty tensors (the reference fails on ``torch.cat([])``, :498); boxes are taken as non-negative
    pixel coordinates (as detectron2 clips them).
    """
    if pairwise_size != 3:
        raise ValueError("only pairwise_size 3 is implemented")
    dev = org_images[0].device
    _need_cuda(*org_images)
    masks = []
    for i, img in enumerate(org_images):
        m = torch.ones(img.shape[-2:], dtype=torch.float32, device=dev)
        removed = int(bottom_pixels_removed * float(img.shape[-2]) / float(img_heights[i]))
        if removed > 0:
            m[-removed:, :] = 0
        masks.append(m)
    images = _pad_stack([x.float() for x in org_images], size_divisibility, 0.0)
    image_masks = _pad_stack(masks, size_divisibility, 0.0)
    stride = mask_out_stride
    start = stride // 2
    Hp, Wp = images.shape[-2:]
    if Hp % stride or Wp % stride:
        raise ValueError("padded image size must be a multiple of mask_out_stride")
    lab = images_lab(images, stride)
    ds_masks = image_masks[:, start::stride, start::stride]
    sim = color_similarity(lab, ds_masks, pairwise_dilation)        # (B, 8, h, w)
    h, w = Hp // stride, Wp // stride
    ys = start + stride * torch.arange(h, device=dev)
    xs = start + stride * torch.arange(w, device=dev)
    out = []
    for b, t in enumerate(targets):
        boxes, labels = _boxes_and_labels(t)
        boxes = boxes.to(dev).float()
        G = boxes.shape[0]
        # python int(): truncation toward zero; slices [y0, y1 + 1) clipped to the padded image
        ib = boxes.trunc().long()
        x0, y0 = ib[:, 0], ib[:, 1]
        x1 = ib[:, 2].clamp(max=Wp - 1)
        y1 = ib[:, 3].clamp(max=Hp - 1)
        in_y = (ys[None] >= y0[:, None]) & (ys[None] <= y1[:, None])        # (G, h)
        in_x = (xs[None] >= x0[:, None]) & (xs[None] <= x1[:, None])        # (G, w)
        box_masks = (in_y[:, :, None] & in_x[:, None, :]).float()
        nonempty_x = (x1 >= x0)[:, None]
        nonempty_y = (y1 >= y0)[:, None]
        # argmax of a box row = its first column (0 for an empty row); W - argmax(flipped) = last + 1 (or W)
        row_on = in_y & nonempty_x
        col_on = in_x & nonempty_y
        left = torch.where(row_on, x0[:, None].float(), 0.0) / stride
        right = torch.where(row_on, (x1 + 1)[:, None].float(), float(Wp)) / stride
        top = torch.where(col_on, y0[:, None].float(), 0.0) / stride
        bottom = torch.where(col_on, (y1 + 1)[:, None].float(), float(Hp)) / stride
        out.append({
            "labels": labels.to(dev),
            "box_masks": box_masks,
            "images_color_similarity": sim[b:b + 1].expand(G, 8, h, w),
            "left_bounds": left.float(), "right_bounds": right.float(),
            "top_bounds": top.float(), "bottom_bounds": bottom.float(),
        })
    return out
