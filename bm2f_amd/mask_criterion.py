"""Mask-supervised Hungarian matcher and set criterion (``SUP_TYPE: "mask"``) on fused HIP point sampling.

Drop-ins for the reference's ``HungarianMatcher`` (mask2former/modeling/matcher.py:479-597), ``SetCriterion``
(modeling/criterion.py:775-955), ``VideoHungarianMatcher`` (mask2former_video/modeling/matcher.py:503-590) and
``VideoSetCriterion`` (mask2former_video/modeling/criterion.py:144-310): same constructor arguments, the
``empty_weight`` buffer, ``__repr__``, ``forward(outputs, targets)`` contracts and loss keys (``loss_ce``,
``loss_mask``, ``loss_dice`` and the ``_i`` aux copies).  Inputs as in the reference: ``pred_logits`` (B, Q, C+1),
``pred_masks`` (B, Q, H, W) or (B, Q, T, H, W) in fp32 / fp16 / bf16 (evaluated in fp32); target dicts with
``labels`` and ``masks`` (G, Ht, Wt) / (G, T, Ht, Wt) (bool, uint8 or float, at their own resolution), and
``box_masks_full`` for ``mask_target_type="box_mask"``.  The image classes also take label-map targets
(``bm2f_amd/label_targets.py``): ``labels``, ``label_map`` (Ht, Wt) and ``ids`` (G,) in place of ``masks``, target g
being ``label_map == ids[g]``; a batch is all dense or all label maps.

Semantics (``point_sample(x, u) = grid_sample(x, 2u - 1, bilinear, zeros, align_corners=False)``):

* matcher: one set of ``num_points`` coordinates per image, shared by its Q predictions and G targets (and, for
  video, by all T frames); ``cost_mask = (sum_k softplus(x_qk) - sum_k x_qk t_gk) / K`` (the reference's
  ``pos . t + neg . (1 - t)``: softplus(-x) - softplus(x) = -x), ``cost_dice = 1 - (2 sum sig(x) t + 1) /
  (sum sig(x) + sum t + 1)``, class cost ``-softmax[:, labels]``; video sums and the divisor run over T K;
* criterion, per head: ``int(num_points * oversample_ratio)`` uniform points per matched mask (video: per matched
  (mask, frame) row) -> uncertainty ``-|x|`` -> the ``int(importance_sample_ratio * num_points)`` most uncertain
  -> plus ``num_points`` minus that fresh uniform points -> ``loss_mask = sum_rows mean_k BCE / num_masks``,
  ``loss_dice = sum_rows (1 - (2 sum sig t + 1) / (sum sig + sum t + 1)) / num_masks`` (detectron2's
  ``get_uncertain_point_coords_with_randomness``);
* the image criterion normalises target coordinates over the batch's padded size (``nested_tensor_from_tensor_list``
  pads bottom / right with zeros); the matcher uses each image's own size.  The pad is never materialised.

Where the work runs on a HIP device (csrc/point_sample.hip): the matching cost of all images of a head is one
``m2f_point_match_cost`` call (no (B, Q, K) tensor, bitwise repeatable) feeding one ``m2f_lsap_batched`` launch;
the oversampling pass is ``m2f_point_uncertainty`` + ``torch.topk``; the losses are the ``m2f_point_loss_fwd`` /
``_bwd`` pair, which reads predictions through a plane index table and targets in place through a pointer table
(no gathered ``pred_masks[src_idx]``, no float copy of the targets) and scatters the gradient with fp32 atomics into
one dense buffer per head.  Label-map targets take the ``_labels`` twins of the match-cost and loss entry points,
which read the map and the ids in place and give bitwise the dense uint8 planes' results; no plane is formed.
``num_masks`` stays a device scalar under torch.distributed; matcher status is checked
with one sync per criterion call (``check_matching = False`` skips it).  Indices are int64 tensors on the masks'
device.

Randomness: every module has a settable ``point_source(kind, shape, device) -> float32 tensor in [0, 1)`` (default
``torch.rand`` on the masks' device), called exactly once per kind per head, in head order (main, aux 0, ...):
``"match"`` (B, K, 2), ``"oversample"`` (N, K * ratio, 2), ``"random"`` (N, K_random, 2; not called when that is 0).
A criterion passes its own source to its matcher unless the matcher has one set.  The distribution is the
reference's; the random stream is not.

On CPU tensors the same classes evaluate the same definition in plain torch (``F.grid_sample``, ``torch.topk``,
scipy).  That is not a fall-back: on a HIP tensor a kernel error raises.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _native
from . import weaksup as ws
from .label_targets import as_label_maps, label_targets_to_masks
from .set_criterion import _class_cost, _Matcher, _SetCriterion, _Targets


def _rand_source(kind, shape, device):
    return torch.rand(shape, device=device)


def point_sample(x, u):
    """x (N, C, H, W), u (N, P, 2) in [0, 1] -> (N, C, P) (detectron2's point_sample, align_corners=False)."""
    return F.grid_sample(x, 2.0 * u[:, :, None] - 1.0, mode="bilinear", padding_mode="zeros",
                         align_corners=False).squeeze(3)


def _logit_tensor(masks):
    """The masks in a dtype the kernels read (fp32 / fp16 / bf16), contiguous."""
    if masks.dtype not in _native.DTYPE_CODES:
        masks = masks.float()
    return masks.contiguous()


class MaskTargets(_Targets):
    """Per-call target tensors shared by the matcher and the mask loss of all decoder heads.  The masks are kept as
    they are (bool viewed as uint8, uint8 or fp32; anything else is converted to fp32 once) and addressed by the
    kernels through pointer tables built here without a host synchronisation."""

    def __init__(self, targets, device, video):
        super().__init__(targets, device)
        self.video = video
        self._planes = {}

    def planes(self, key="masks"):
        """dict: ``list`` per-image planes (G, [T,] Ht, Wt), ``code`` 0 uint8 / 1 fp32, ``sizes`` (Ht, Wt) per
        image, ``pad`` the batch maximum, and on a HIP device ``match`` (B, 4) int64 [pointer, G, Ht, Wt] and
        ``rows`` (B, 4) int64 [pointer, plane bytes, Ht, Wt].

        Label-map targets under ``"masks"``: on a HIP device ``code`` 2, ``list`` the maps (Ht, Wt), ``label_bytes``
        their item size, ``ids`` the batch's ids (sum G,) int32, ``match`` (B, 5) [map pointer, G, Ht, Wt, pointer
        to the image's ids] and ``rows`` (B, 5) [map pointer, 0, Ht, Wt, offset of the image's ids]; on the CPU the
        dense uint8 planes made from the maps."""
        hit = self._planes.get(key)
        if hit is not None:
            return hit
        if key == "masks" and any("label_map" in t for t in self._targets):
            out = self._planes[key] = self._label_planes()
            return out
        raw = [t[key].to(self.device) for t in self._targets]
        nd = 4 if self.video else 3
        for b, m in enumerate(raw):
            if m.dim() != nd or m.shape[0] != self.G[b]:
                raise ValueError(f"targets[{b}][{key!r}] must be (G, {'T, ' if self.video else ''}H, W) with one "
                                 "mask per label")
        as_u8 = all(m.dtype in (torch.bool, torch.uint8) for m in raw)
        if as_u8:
            lst = [(m.view(torch.uint8) if m.dtype == torch.bool else m).contiguous() for m in raw]
        else:
            lst = [m.to(torch.float32).contiguous() for m in raw]
        sizes = [(int(m.shape[-2]), int(m.shape[-1])) for m in lst]
        out = {"list": lst, "code": 0 if as_u8 else 1, "sizes": sizes,
               "pad": (max((s[0] for s in sizes), default=0), max((s[1] for s in sizes), default=0))}
        if self.cuda:
            item = 1 if as_u8 else 4
            # an image without targets has no storage to point at: null pointer, skipped by the kernels
            ptr = [m.data_ptr() if m.numel() else 0 for m in lst]
            out["match"] = ws.h2d([v for b in range(self.B) for v in (ptr[b], self.G[b], *sizes[b])], self.device,
                                  torch.int64).view(self.B, 4)
            out["rows"] = ws.h2d([v for b in range(self.B) for v in (ptr[b], sizes[b][0] * sizes[b][1] * item,
                                                                      *sizes[b])], self.device,
                                 torch.int64).view(self.B, 4)
        self._planes[key] = out
        return out

    def _label_planes(self):
        if self.video:
            raise ValueError("label-map targets are for images; the video classes take dense masks")
        for b, t in enumerate(self._targets):
            if "label_map" not in t or "masks" in t:
                raise ValueError(f"targets[{b}]: a batch is either all dense masks or all label maps")
            if "ids" not in t or t["ids"].dim() != 1 or t["ids"].shape[0] != self.G[b]:
                raise ValueError(f"targets[{b}]['ids'] must be (G,) with one id per label")
        if not self.cuda:
            dense = [label_targets_to_masks(t).view(torch.uint8) for t in self._targets]
            sizes = [(int(m.shape[-2]), int(m.shape[-1])) for m in dense]
            return {"list": dense, "code": 0, "sizes": sizes,
                    "pad": (max((s[0] for s in sizes), default=0), max((s[1] for s in sizes), default=0))}
        maps = as_label_maps([t["label_map"].to(self.device) for t in self._targets])
        ids = torch.cat([t["ids"].to(self.device, torch.int32) for t in self._targets]) if self.B else None
        sizes = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
        item = maps[0].element_size() if maps else 1
        # an image without targets or pixels has nothing to point at: null pointer, skipped by the kernels
        ptr = [m.data_ptr() if m.numel() and self.G[b] else 0 for b, m in enumerate(maps)]
        id_ptr = [ids.data_ptr() + 4 * self.offsets[b] if self.G[b] else 0 for b in range(self.B)]
        return {"list": maps, "code": 2, "label_bytes": item, "ids": ids, "sizes": sizes,
                "pad": (max((s[0] for s in sizes), default=0), max((s[1] for s in sizes), default=0)),
                "match": ws.h2d([v for b in range(self.B) for v in (ptr[b], self.G[b], *sizes[b], id_ptr[b])],
                                self.device, torch.int64).view(self.B, 5),
                "rows": ws.h2d([v for b in range(self.B) for v in (ptr[b], 0, *sizes[b], self.offsets[b])],
                               self.device, torch.int64).view(self.B, 5)}


# ------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------
def match_cost(masks, coords, tgt_table, tgt_code, Gm, cost_class=None, w_class=0.0, w_mask=1.0, w_dice=1.0,
               label_bytes=0):
    """``m2f_point_match_cost``: masks (B, Q, H, W) or (B, Q, T, H, W), coords (B, K, 2) fp32, tgt_table (B, 4)
    int64 -> (B, Q, Gm) fp32 weighted cost.  ``tgt_code`` 2: label-map targets of ``label_bytes`` per label through
    ``m2f_point_match_cost_labels`` (images only, tgt_table (B, 5)).  The caller keeps the target tensors alive."""
    ws._need_cuda(masks, coords, tgt_table, cost_class)
    x = _logit_tensor(masks)
    B, Q = x.shape[:2]
    T = x.shape[2] if x.dim() == 5 else 1
    H, W = x.shape[-2:]
    K = coords.shape[1]
    c = coords.to(torch.float32).contiguous()
    labels = tgt_code == 2
    if labels and x.dim() == 5:
        raise ValueError("label-map targets are for images")
    if c.shape != (B, K, 2) or tgt_table.shape != (B, 5 if labels else 4) or tgt_table.dtype != torch.int64:
        raise ValueError("coords must be (B, K, 2) and the target table (B, 4) int64, (B, 5) for label maps")
    cc = None
    if cost_class is not None:
        cc = cost_class.to(torch.float32).contiguous()
        if cc.shape != (B, Q, Gm):
            raise ValueError("cost_class must be (B, Q, Gm)")
    n = _native.query("m2f_point_match_workspace", B, T, Q, Gm, K)
    work = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    cost = torch.empty((B, Q, Gm), dtype=torch.float32, device=x.device)
    tail = (Gm, _native.ptr(cc), w_class, w_mask, w_dice, work.data_ptr(), n, cost.data_ptr(), _native.stream(x))
    dt = _native.dtype_code(x.dtype, "mask criterion")
    if labels:
        _native.call("m2f_point_match_cost_labels", x.data_ptr(), dt, B, Q, H, W, c.data_ptr(), K,
                     tgt_table.contiguous().data_ptr(), label_bytes, *tail)
    else:
        _native.call("m2f_point_match_cost", x.data_ptr(), dt, B, Q, T, H, W, c.data_ptr(), K,
                     tgt_table.contiguous().data_ptr(), tgt_code, *tail)
    return cost


def point_uncertainty(masks, plane, coords):
    """``-|point_sample(masks.view(-1, H, W)[plane[r]], coords[r])|``: plane (R,) int64, coords (R, P, 2) ->
    (R, P) fp32."""
    ws._need_cuda(masks, plane, coords)
    x = _logit_tensor(masks)
    H, W = x.shape[-2:]
    R, P = coords.shape[:2]
    c = coords.to(torch.float32).contiguous()
    out = torch.empty((R, P), dtype=torch.float32, device=x.device)
    _native.call("m2f_point_uncertainty", x.data_ptr(), _native.dtype_code(x.dtype, "mask criterion"),
                 x.numel() // (H * W), H, W, plane.contiguous().data_ptr(), R, c.data_ptr(), P, out.data_ptr(),
                 _native.stream(x))
    return out


class PointLossSums(Function):
    """Per row r: sum_k BCE(x, t), sum sig(x) t, sum sig(x), sum t at the row's K points; x sampled from plane
    ``plane[r]`` of masks, t from the row's target (tgt_rows (R, 5) int64: pointer, Ht, Wt, Hn, Wn; for label-map
    targets, ``tgt_code`` 2, (R, 6): map pointer, id, Ht, Wt, Hn, Wn and ``label_bytes`` per label).  Differentiable
    in masks: the backward pass re-samples (only the tables and coordinates are saved) and scatters with fp32
    atomics into one dense gradient."""

    @staticmethod
    def forward(ctx, masks, plane, coords, tgt_rows, tgt_code, keep, label_bytes=0):
        H, W = masks.shape[-2:]
        R, K = coords.shape[:2]
        chunks = _native.load().m2f_point_loss_chunks(K)
        part = torch.empty((R, max(chunks, 1), 4), dtype=torch.float32, device=masks.device)
        n_planes = masks.numel() // (H * W)
        # (entry point suffix, its target code): the dense dtype code, or the bytes per label
        ctx.target = ("_labels", label_bytes) if tgt_code == 2 else ("", tgt_code)
        _native.call("m2f_point_loss_fwd" + ctx.target[0], masks.data_ptr(),
                     _native.dtype_code(masks.dtype, "mask criterion"), n_planes, H, W, plane.data_ptr(), R,
                     coords.data_ptr(), K, tgt_rows.data_ptr(), ctx.target[1], part.data_ptr(), _native.stream(masks))
        ctx.save_for_backward(masks, plane, coords, tgt_rows)
        ctx.keep = keep                      # the target tensors the pointer table refers to
        sums = part.sum(1)
        bce, inter, sig, tsum = sums.unbind(1)
        ctx.mark_non_differentiable(tsum)
        return bce, inter, sig, tsum

    @staticmethod
    def backward(ctx, g_bce, g_inter, g_sig, g_t):
        masks, plane, coords, tgt_rows = ctx.saved_tensors
        H, W = masks.shape[-2:]
        R, K = coords.shape[:2]
        g = torch.stack([g_bce, g_inter, g_sig], 1).to(torch.float32).contiguous()
        grad = torch.zeros(masks.shape, dtype=torch.float32, device=masks.device)
        _native.call("m2f_point_loss_bwd" + ctx.target[0], masks.data_ptr(),
                     _native.dtype_code(masks.dtype, "mask criterion"), grad.numel() // (H * W), H, W, plane.data_ptr(),
                     R, coords.data_ptr(), K, tgt_rows.data_ptr(), ctx.target[1], g.data_ptr(), grad.data_ptr(),
                     _native.stream(masks))
        return grad.to(masks.dtype), None, None, None, None, None, None


def point_loss_sums(masks, plane, coords, tgt_rows, tgt_code, keep=None, label_bytes=0):
    ws._need_cuda(masks, plane, coords, tgt_rows)
    fields = 6 if tgt_code == 2 else 5
    if tgt_rows.dtype != torch.int64 or tgt_rows.shape != (coords.shape[0], fields) or plane.dtype != torch.int64:
        raise ValueError("plane must be (R,) int64 and the target table (R, 5) int64, (R, 6) for label maps")
    return PointLossSums.apply(_logit_tensor(masks), plane.contiguous(), coords.to(torch.float32).contiguous(),
                               tgt_rows.contiguous(), tgt_code, keep, label_bytes)


# ------------------------------------------------------------------------------------------------------------
# matchers
# ------------------------------------------------------------------------------------------------------------
class HungarianMatcher(_Matcher):
    """Reference: mask2former/modeling/matcher.py:479-597 (same arguments; no buffers)."""

    _video = False

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        self.num_points = num_points
        self.point_source = None     # None: the caller's (a criterion's) source, else torch.rand

    @torch.no_grad()
    def cost_matrix(self, outputs, tg: MaskTargets, coords) -> torch.Tensor:
        """(B, Q, Gm) fp32 matching cost of every image / clip at coords (B, K, 2) (columns >= G_b: padding)."""
        logits, masks = outputs["pred_logits"], outputs["pred_masks"]
        B, Q = logits.shape[:2]
        Gm = tg.Gm
        pl = tg.planes("masks")
        c_class = _class_cost(logits, tg.labels_padded())
        if tg.cuda:
            return match_cost(masks, coords, pl["match"], pl["code"], Gm, c_class, self.cost_class, self.cost_mask,
                              self.cost_dice, label_bytes=pl.get("label_bytes", 0))
        C = torch.zeros((B, Q, Gm), dtype=torch.float32)
        for b in range(B):
            G = tg.G[b]
            if G == 0:
                continue
            x, t = masks[b].float(), pl["list"][b].float()
            if not self._video:
                x, t = x[:, None], t[:, None]
            x = point_sample(x, coords[b:b + 1].expand(Q, -1, -1)).flatten(1)           # (Q, T*K)
            t = point_sample(t, coords[b:b + 1].expand(G, -1, -1)).flatten(1)           # (G, T*K)
            s = x.sigmoid()
            c_mask = (F.softplus(x).sum(1)[:, None] - x @ t.t()) / x.shape[1]
            c_dice = 1 - (2 * (s @ t.t()) + 1) / (s.sum(1)[:, None] + t.sum(1)[None] + 1)
            C[b, :, :G] = self.cost_mask * c_mask + self.cost_class * c_class[b, :, :G] + self.cost_dice * c_dice
        return C

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets, prepared: MaskTargets | None = None, point_source=None):
        masks = outputs["pred_masks"]
        if masks.dim() != (5 if self._video else 4):
            raise ValueError("pred_masks must be (B, Q, T, H, W)" if self._video else "pred_masks must be (B, Q, H, W)")
        tg = prepared or MaskTargets(targets, masks.device, self._video)
        source = self.point_source or point_source or _rand_source
        # drawn before the no-target return: one "match" draw per head whatever the targets
        coords = source("match", (outputs["pred_logits"].shape[0], self.num_points, 2), masks.device)
        return self._assign(outputs, tg, coords)

    @torch.no_grad()
    def forward(self, outputs, targets, prepared: MaskTargets | None = None, point_source=None):
        return self.memory_efficient_forward(outputs, targets, prepared, point_source)

    def __repr__(self, _repr_indent=4):
        return self._repr(("cost_class", "cost_mask", "cost_dice"), _repr_indent)


class VideoHungarianMatcher(HungarianMatcher):
    """Reference: mask2former_video/modeling/matcher.py:503-590: the same K points in every one of the T frames,
    sums and the divisor over T K."""

    _video = True


# ------------------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------------------
class SetCriterion(_SetCriterion):
    """Reference: mask2former/modeling/criterion.py:775-955; ``losses`` is any subset of "labels", "masks"."""

    _video = False
    _matcher_class = HungarianMatcher
    _loss_table = {"labels": "loss_labels", "masks": "loss_masks"}

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                 importance_sample_ratio, mask_target_type="mask"):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, losses)
        self.num_points = num_points
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        if mask_target_type not in ("mask", "box_mask"):
            raise ValueError('mask_target_type must be "mask" or "box_mask"')
        self.mask_target_type = mask_target_type
        self.point_source = _rand_source

    # -- losses ----------------------------------------------------------------------------------------------
    def _target_key(self):
        return "box_masks_full" if self.mask_target_type == "box_mask" else "masks"

    def _sample_points(self, uncertainty, R, device):
        """get_uncertain_point_coords_with_randomness; ``uncertainty(coords (R, P, 2)) -> (R, P)``."""
        n_over = int(self.num_points * self.oversample_ratio)
        n_unc = int(self.importance_sample_ratio * self.num_points)
        n_rand = self.num_points - n_unc
        over = self.point_source("oversample", (R, n_over, 2), device)
        idx = torch.topk(uncertainty(over), k=n_unc, dim=1)[1]
        coords = torch.gather(over, 1, idx[:, :, None].expand(-1, -1, 2))
        if n_rand > 0:
            coords = torch.cat([coords, self.point_source("random", (R, n_rand, 2), device)], dim=1)
        return coords

    def loss_masks(self, outputs, targets, indices, num_masks):
        masks = outputs["pred_masks"]
        dev = masks.device
        tg = self._targets(targets, dev)
        batch_idx, src_idx = self._get_src_permutation_idx(indices)
        N = int(batch_idx.shape[0])
        if N == 0 or self.num_points == 0:
            zero = masks.flatten()[:0].float().sum()  # no matched mask: zero, still connected to pred_masks
            return {"loss_mask": zero, "loss_dice": zero}
        tgt_idx = torch.cat([j for (_, j) in indices])
        pl = tg.planes(self._target_key())
        Q = masks.shape[1]
        T = masks.shape[2] if self._video else 1
        if tg.cuda:
            x = _logit_tensor(masks)
            frames = torch.arange(T, device=dev)
            plane = ((batch_idx * Q + src_idx)[:, None] * T + frames).reshape(-1)                    # (R,)
            info = pl["rows"][batch_idx]                                                            # (N, 4)
            ptr = info[:, :1] + (tgt_idx[:, None] * T + frames) * info[:, 1:2]                      # (N, T)
            size = info[:, None, 2:4].expand(N, T, 2)
            # the image criterion samples targets zero-padded to the batch maximum; video clips share one size
            norm = size if self._video else torch.tensor(pl["pad"], dtype=torch.int64).pin_memory().to(
                dev, non_blocking=True).expand(N, T, 2)
            cols = [ptr[:, :, None], size, norm]
            if pl["code"] == 2:   # every row of an image points at its map; the row's target is its id
                cols.insert(1, pl["ids"][info[:, 4] + tgt_idx].long()[:, None, None])
            rows = torch.cat(cols, 2).reshape(N * T, len(cols) + 2)
            with torch.no_grad():
                coords = self._sample_points(lambda u: point_uncertainty(x.detach(), plane, u), N * T, dev)
            bce, inter, sig, tsum = point_loss_sums(x, plane, coords, rows, pl["code"],
                                                    keep=(pl["list"], pl.get("ids")),
                                                    label_bytes=pl.get("label_bytes", 0))
        else:
            src = masks[batch_idx, src_idx].float()
            Hp, Wp = pl["pad"]
            tgt = []
            for b, (_, j) in enumerate(indices):
                m = pl["list"][b][j].float()
                tgt.append(m if self._video else F.pad(m, (0, Wp - m.shape[-1], 0, Hp - m.shape[-2])))
            tgt = torch.cat(tgt)
            src = (src.flatten(0, 1) if self._video else src)[:, None]                              # (R, 1, H, W)
            tgt = (tgt.flatten(0, 1) if self._video else tgt)[:, None]
            with torch.no_grad():
                coords = self._sample_points(lambda u: -point_sample(src, u)[:, 0].abs(), src.shape[0], dev)
                t = point_sample(tgt, coords)[:, 0]
            xk = point_sample(src, coords)[:, 0]
            s = xk.sigmoid()
            bce = F.binary_cross_entropy_with_logits(xk, t, reduction="none").sum(1)
            inter, sig, tsum = (s * t).sum(1), s.sum(1), t.sum(1)
        loss_mask = (bce / coords.shape[1]).sum() / num_masks
        loss_dice = (1 - (2 * inter + 1) / (sig + tsum + 1)).sum() / num_masks
        return {"loss_mask": loss_mask, "loss_dice": loss_dice}

    # -- driver ----------------------------------------------------------------------------------------------
    def _make_targets(self, targets, device):
        return MaskTargets(targets, device, self._video)

    def _matcher_kwargs(self):
        return {"point_source": self.point_source}

    def _repr_body(self):
        return super()._repr_body() + [f"num_points: {self.num_points}",
                                       f"oversample_ratio: {self.oversample_ratio}",
                                       f"importance_sample_ratio: {self.importance_sample_ratio}"]


class VideoSetCriterion(SetCriterion):
    """Reference: mask2former_video/modeling/criterion.py:144-310 (eight-argument constructor): every one of the
    N T (matched mask, frame) rows is its own mask with its own points; targets are ``t["masks"]``."""

    _video = True

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                 importance_sample_ratio):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                         importance_sample_ratio, "mask")
