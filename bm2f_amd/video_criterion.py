"""Box-supervised video matcher and set criterion (projection, spatial colour-pairwise and temporal-pairwise
losses) on the GPU.

Drop-ins for the reference's ``VideoHungarianMatcherProj`` / ``VideoHungarianMatcherProjPair``
(mask2former_video/modeling/matcher.py:249-501) and ``VideoSetCriterionProj`` / ``...ProjSpatPair`` /
``...ProjSpatPairTempPair`` (modeling/criterion_proj.py, criterion_proj_spatpair.py,
criterion_proj_spatpair_temppair.py): same constructor arguments, buffers (``empty_weight``, ``_iter``: checkpoints
load), ``forward(outputs, targets)`` contracts and loss keys (``loss_ce``, ``loss_mask_projection``,
``loss_mask_spatial_pairwise``, ``loss_mask_temporal_pairwise`` and the ``_i`` aux copies).  Inputs as in the
reference: ``pred_logits`` (B, Q, K+1), ``pred_masks`` (B, Q, T, H, W) in fp32 / fp16 / bf16 (all arithmetic is
fp32); target dicts with ``labels``, ``box_masks`` (G, T, H, W), ``color_similarities`` (G, T, 8, H, W) and
``temporal_pairs`` (the reference's nested ``[[(curr, next)] * (T-1)] * G`` XY lists, or the
:class:`bm2f_amd.weaksup.MinedPairs` that :func:`bm2f_amd.weaksup.temporal_pairs` returns).

The semantics are the video reference's, which differ from the image criterion (criterion.py):

* matcher projection cost: dice over the concatenation of all T frames' axis maxima (matcher.py:43-54);
* matcher pairwise cost: per frame numerator / per-(target, frame) denominator clamp(min=1), mean over T
  (matcher.py:235-246);
* spatial pairwise loss: per (instance, frame) num / den.clamp(min=1), mean over T, sum over instances,
  / num_masks, times the warm-up factor (criterion_proj_spatpair.py:21-37);
* projection loss: dice per (instance, frame) row with eps 1e-5 (criterion_proj.py:18-47);
* temporal pairwise loss: sum of s over every pair of every matched instance / max(#pairs, 1), times the warm-up
  factor, not divided by num_masks (criterion_proj_spatpair_temppair.py:25-30, :269-334);
* ``_iter``: the criterion increments at the end of ``forward`` (its first call sees factor 0), the matcher at the
  start.

Where the work runs on a HIP device: frames are treated as images, so one fp32 cast-and-permute of ``pred_masks``
to (B*T, Q, H, W) feeds ``m2f_pairwise_match_cost`` (per-frame numerators and both axis maxima in one read); all
B clips are solved by one ``m2f_lsap_batched`` launch per head; the spatial loss is ``PairwiseSums`` on the matched
masks viewed as (N*T, H, W) rows; the temporal loss is the ``m2f_temporal_pairs_fwd`` / ``_bwd`` pair on pairs
packed once per call.  The target-side tensors are built once per ``forward`` for all heads.  There is no
``.item()`` per head: ``_iter`` is mirrored on the host, and matcher status plus pair validity are checked with one
sync per call (``check_matching = False`` skips it).

On CPU tensors the same classes evaluate the same definition in plain torch (scipy for the assignment), so the
host logic is testable without a GPU.  That is not a fall-back: on a HIP tensor a kernel error raises.

The matcher and the targets also serve the image criterion (criterion.py) as the one-frame case: targets and masks
without a frame axis.  The driver shared with the other criterion families is set_criterion.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pad_sequence

from . import weaksup as ws
from .set_criterion import _bit_planes, _class_cost, _dice_cost, _IterMirror, _Matcher, _SetCriterion, _Targets


def _neighbours(x, d):
    """(N, H, W) -> (N, 8, H, W): the 3x3 dilated taps minus the centre, zero outside (unfold_wo_center)."""
    N, H, W = x.shape
    xp = F.pad(x, (d, d, d, d))
    return torch.stack([xp[:, ky * d:ky * d + H, kx * d:kx * d + W]
                        for ky in range(3) for kx in range(3) if (ky, kx) != (1, 1)], 1)


def _pred_similarity(x, d):
    """calculate_pred_similaries_video (criterion_proj_spatpair.py:45-71) on (N, H, W) rows -> (N, 8, H, W)."""
    lf, lb = F.logsigmoid(x), F.logsigmoid(-x)
    u = lf[:, None] + _neighbours(lf, d)
    v = lb[:, None] + _neighbours(lb, d)
    m = torch.max(u, v)
    return -(torch.log(torch.exp(u - m) + torch.exp(v - m)) + m)


def _bits_torch(sim, thr):
    k = torch.arange(8, device=sim.device).view(1, 8, 1, 1)
    return ((sim >= thr).to(torch.int32) << k).sum(1).to(torch.uint8)


def _frames_side_by_side(v, B, T):
    """Per-frame rows (B*T, N, L) -> (B, N, T*L); one frame is returned as it is."""
    if T == 1:
        return v
    return v.view(B, T, v.shape[1], -1).transpose(1, 2).reshape(B, v.shape[1], -1)


class VideoWeakTargets(_Targets):
    """Per-call target tensors shared by the matcher and every loss of all decoder heads: padded boxes, neighbour
    bits, extents, pairwise denominators and the packed temporal pairs.  Targets without a frame axis (``box_masks``
    (G, H, W), similarity (G, 8, H, W): criterion.WeakTargets) are clips of one frame."""

    _sim_key = "color_similarities"

    def __init__(self, targets, device, thresh, need_sim=True):
        super().__init__(targets, device)
        self.thresh = thresh
        self.box_list = [t["box_masks"].to(device=device, dtype=torch.float32) for t in targets]  # (G, [T,] H, W)
        self.T, self.H, self.W = 0, 0, 0
        if self.box_list:
            self.T = int(self.box_list[0].shape[1]) if self.box_list[0].dim() == 4 else 1
            self.H, self.W = (int(v) for v in self.box_list[0].shape[-2:])
        T, H, W = self.T, self.H, self.W
        self.box_all = torch.cat(self.box_list).reshape(-1, H, W).contiguous() if self.box_list else None  # (Gt*T,..)
        self.bits = self.sim_list = None
        self.shared = True
        if need_sim:
            sims = [t[self._sim_key] for t in targets]                                           # (G, [T,] 8, H, W)
            self.shared = all(s.shape[0] <= 1 or s.stride(0) == 0 for s in sims)
            to_bits = ws.threshold_bits if self.cuda else _bits_torch
            if self.shared:
                # the frame's one map shared across instances -> bits per (clip, frame)
                one = tuple(self.box_list[0].shape[1:-2]) + (8, H, W)
                img = [s[0] if s.shape[0] else s.new_zeros(one) for s in sims]
                img = torch.stack([s.to(device=device, dtype=torch.float32) for s in img])       # (B, [T,] 8, H, W)
                self.bits = to_bits(img.reshape(self.B * T, 8, H, W).contiguous(), thresh)       # (B*T, H, W)
            else:
                self.sim_list = [s.to(device=device, dtype=torch.float32) for s in sims]
                sim_all = torch.cat(self.sim_list).reshape(-1, 8, H, W)
                self.bits = to_bits(sim_all.contiguous(), thresh) if sim_all.shape[0] else None  # (Gt*T, H, W)
        self._box_padded = self._match_aux = self._pairs = None

    def box_padded(self):
        """The boxes as frames-as-images (B*T, Gm, H, W), zero beyond a clip's G."""
        if self._box_padded is None:
            box = pad_sequence(self.box_list, batch_first=True).view(self.B, self.Gm, self.T, self.H, self.W)
            self._box_padded = box.transpose(1, 2).reshape(self.B * self.T, self.Gm, self.H, self.W)
        return self._box_padded

    def match_aux(self):
        """Matcher-side constants of the targets: box axis projections, the pairwise normaliser
        sum_p box_g(p) popcount(bits(p)) (shared similarity) and the per-frame target counts."""
        if self._match_aux is None:
            box = self.box_padded()
            B, Gm, T = self.B, self.Gm, self.T
            aux = {"box_x": _frames_side_by_side(box.amax(3), B, T),        # (B, Gm, T*H)
                   "box_y": _frames_side_by_side(box.amax(2), B, T)}        # (B, Gm, T*W)
            if self.cuda:
                aux["gcount"] = ws.h2d(np.repeat(self.G, T).tolist(), self.device)
                aux["extents"] = ws.box_extents(box)
            if self.shared and self.bits is not None:
                tsum = _bit_planes(self.bits).sum(1, dtype=torch.float32).view(B * T, 1, -1)       # (B*T, 1, HW)
                aux["pair_den"] = (box.view(B * T, Gm, -1) * tsum).sum(-1).clamp(min=1.0)          # (B*T, Gm)
            self._match_aux = aux
        return self._match_aux

    def pairs(self):
        if self._pairs is None:
            per_clip = [t["temporal_pairs"] for t in self._targets]
            for b, clip in enumerate(per_clip):
                if len(clip) != self.G[b]:
                    raise ValueError("temporal_pairs needs one entry per target")
            self._pairs = ws.pack_temporal_pairs(per_clip, self.T, self.H, self.W, self.device)
        return self._pairs


class VideoHungarianMatcherProjPair(_Matcher):
    """Reference: mask2former_video/modeling/matcher.py:249-393 (same arguments and ``_iter`` buffer);
    ``cost_pairwise = 0`` is ``VideoHungarianMatcherProj`` (:396-501).  Masks without a frame axis, (B, Q, H, W),
    are one-frame clips: the image matcher (criterion.HungarianMatcherProjPair)."""

    _repr_fields = ("cost_class", "cost_projection", "cost_pairwise", "pairwise_size", "pairwise_dilation",
                    "pairwise_color_thresh")

    def __init__(self, cost_class: float = 1, cost_projection: float = 1, cost_pairwise: float = 1,
                 pairwise_size: int = 3, pairwise_dilation: int = 2, pairwise_color_thresh: float = 0.3,
                 pairwise_warmup_iters: int = 10000, _persistent_iter: bool = True):
        super().__init__()
        self.cost_class = cost_class
        self.cost_projection = cost_projection
        self.cost_pairwise = cost_pairwise
        self.pairwise_size = pairwise_size
        self.pairwise_dilation = pairwise_dilation
        self.pairwise_color_thresh = pairwise_color_thresh
        self.pairwise_warmup_iters = pairwise_warmup_iters
        assert cost_class != 0 or cost_projection != 0 or cost_pairwise != 0, "all costs cant be 0"
        if pairwise_size != 3:
            raise ValueError("only pairwise_size 3 is implemented")
        self.register_buffer("_iter", torch.zeros([1]), persistent=_persistent_iter)
        self._iter_host = _IterMirror(self)

    def _prepare(self, targets, device):
        return VideoWeakTargets(targets, device, self.pairwise_color_thresh, need_sim=self.cost_pairwise != 0)

    @torch.no_grad()
    def cost_matrix(self, outputs, tg: VideoWeakTargets, warm: float) -> torch.Tensor:
        """(B, Q, Gm) fp32 matching cost of every clip (columns >= G_b are padding)."""
        logits, masks = outputs["pred_logits"], outputs["pred_masks"]
        B, Q = masks.shape[:2]
        T, H, W = tg.T, *masks.shape[-2:]
        box = tg.box_padded()
        aux = tg.match_aux()
        Gm = tg.Gm
        c_class = _class_cost(logits, tg.labels_padded())
        if masks.dim() == 4:
            x = masks.float().contiguous()          # an image: fp32 contiguous masks are read in place
        else:
            # frames as images: the one fp32 cast-and-permute of the masks
            x = torch.empty((B, T, Q, H, W), dtype=torch.float32, device=masks.device)
            x = x.copy_(masks.transpose(1, 2)).view(B * T, Q, H, W)
        want_pair = self.cost_pairwise != 0 and warm != 0
        pair = None
        if tg.cuda and tg.shared and tg.bits is not None:
            # one pass: per-frame pairwise numerators and both axis projections
            num, sx, sy = ws.match_cost(x, tg.bits, box, aux["gcount"], self.pairwise_dilation, aux["extents"])
            pair = num / aux["pair_den"][:, None, :]
            if T > 1:
                pair = pair.view(B, T, Q, Gm).mean(1)
        else:
            sx, sy = x.amax(3), x.amax(2)
            if want_pair:
                pair = self._pairwise_cost_general(x, tg)
        c_proj = _dice_cost(_frames_side_by_side(sx, B, T), aux["box_x"]) + \
            _dice_cost(_frames_side_by_side(sy, B, T), aux["box_y"])
        C = self.cost_class * c_class + self.cost_projection * c_proj
        if want_pair:
            C = C + self.cost_pairwise * (pair * warm)
        return C

    def _pairwise_cost_general(self, x, tg):
        """Per-frame s (Q, 8HW) x T (8HW, G) / den, mean over frames (matcher.py:235-246); the similarity map
        of each (target, frame) is its own (or, on CPU, the shared one expanded)."""
        BT, Q, H, W = x.shape
        B, T = tg.B, tg.T
        d = self.pairwise_dilation
        out = x.new_zeros((B, Q, tg.Gm))
        for b in range(B):
            G = tg.G[b]
            if G == 0:
                continue
            box = tg.box_list[b].view(G, T, H, W)
            sim = None if tg.shared else tg.sim_list[b].view(G, T, 8, H, W)
            for t in range(T):
                xf = x[b * T + t].contiguous()
                s = (ws.pairwise_planes(xf, d) if tg.cuda else _pred_similarity(xf, d)).view(Q, -1)
                if tg.shared:
                    on = _bit_planes(tg.bits[b * T + t][None]).float().expand(G, 8, H, W)
                else:
                    on = (sim[:, t] >= tg.thresh).float()
                tt = (on * box[:, t, None]).reshape(G, -1)
                out[b, :, :G] += (s @ tt.t()) / tt.sum(1)[None].clamp(min=1.0)
        return out.div_(T) if T > 1 else out

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets, prepared: VideoWeakTargets | None = None):
        tg = prepared or self._prepare(targets, outputs["pred_masks"].device)
        warm = min(self._iter_host.value / float(self.pairwise_warmup_iters), 1.0)
        return self._assign(outputs, tg, warm)

    @torch.no_grad()
    def forward(self, outputs, targets, prepared: VideoWeakTargets | None = None):
        self._iter_host.step(self._iter)
        return self.memory_efficient_forward(outputs, targets, prepared)

    def __repr__(self, _repr_indent=4):
        return self._repr(self._repr_fields, _repr_indent)


class VideoHungarianMatcherProj(VideoHungarianMatcherProjPair):
    """Reference: matcher.py:396-501 (class and projection costs only; no ``_iter`` in its state dict)."""

    _repr_fields = ("cost_class", "cost_projection")

    def __init__(self, cost_class: float = 1, cost_projection: float = 1):
        assert cost_class != 0 or cost_projection != 0, "all costs cant be 0"
        super().__init__(cost_class, cost_projection, 0, _persistent_iter=False)


class VideoSetCriterionProjSpatPairTempPair(_SetCriterion):
    """Reference: criterion_proj_spatpair_temppair.py:72-406; ``losses`` is any subset of "labels",
    "projection_masks", "spatial_pairwise", "temporal_pairwise"."""

    _matcher_class = VideoHungarianMatcherProjPair
    _loss_table = {"labels": "loss_labels", "projection_masks": "loss_projection_masks",
                   "spatial_pairwise": "loss_spatial_pairwise", "temporal_pairwise": "loss_temporal_pairwise"}

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, pairwise_size, pairwise_dilation,
                 pairwise_color_thresh, pairwise_warmup_iters, losses):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, losses)
        self.pairwise_size = pairwise_size
        self.pairwise_dilation = pairwise_dilation
        self.pairwise_color_thresh = pairwise_color_thresh
        self.pairwise_warmup_iters = pairwise_warmup_iters
        if pairwise_size != 3:
            raise ValueError("only pairwise_size 3 is implemented")
        self.register_buffer("_iter", torch.zeros([1]))
        self._iter_host = _IterMirror(self)

    # -- losses ------------------------------------------------------------------------------------------
    @staticmethod
    def _zero(device):
        return torch.tensor([0], dtype=torch.float32, device=device)

    def _warm(self):
        return min(self._iter_host.peek(self._iter) / float(self.pairwise_warmup_iters), 1.0)

    def loss_projection_masks(self, outputs, targets, indices, num_masks):
        tg, src, flat = self._matched(outputs, targets, indices)
        if src.shape[0] == 0:
            return {"loss_mask_projection": self._zero(src.device)}
        p = src.sigmoid().flatten(0, 1)                       # (N*T, H, W); sigmoid before max, as the reference
        box = tg.box_all.view(-1, tg.T, tg.H, tg.W)[flat].flatten(0, 1)
        y = p.max(dim=2)[0]
        x = p.max(dim=1)[0]
        with torch.no_grad():
            by = box.max(dim=2)[0]
            bx = box.max(dim=1)[0]

        def dice(a, t):
            inter = (a * t).sum(dim=1)
            union = (a ** 2.0).sum(dim=1) + (t ** 2.0).sum(dim=1) + 1e-5
            return 1. - (2 * inter / union)

        return {"loss_mask_projection": (dice(x, bx) + dice(y, by)).sum() / num_masks}

    def loss_spatial_pairwise(self, outputs, targets, indices, num_masks):
        tg, src, flat = self._matched(outputs, targets, indices)
        N, T, H, W = src.shape
        if N == 0:
            return {"loss_mask_spatial_pairwise": self._zero(src.device)}
        frames = torch.arange(T, device=src.device)
        box_row = (flat[:, None] * T + frames).reshape(-1)                      # rows of box_all (Gt*T, H, W)
        if tg.shared:
            clip = self._get_src_permutation_idx(indices)[0]
            t_row = (clip[:, None] * T + frames).reshape(-1)                    # rows of bits (B*T, H, W)
        else:
            t_row = box_row
        rows = src.view(N * T, H, W)
        if tg.cuda:
            num, den = ws.pairwise_sums(rows, tg.bits, t_row.to(torch.int32).contiguous(), tg.box_all,
                                        box_row.to(torch.int32).contiguous(), self.pairwise_dilation)
        else:
            on = _bit_planes(tg.bits[t_row]).float() * tg.box_all[box_row][:, None]
            num = (_pred_similarity(rows, self.pairwise_dilation) * on).flatten(1).sum(1)
            den = on.flatten(1).sum(1)
        loss = (num / den.clamp(min=1.0)).view(N, T).mean(1).sum() / num_masks
        return {"loss_mask_spatial_pairwise": loss * self._warm()}

    def loss_temporal_pairwise(self, outputs, targets, indices, num_masks):
        tg, src, flat = self._matched(outputs, targets, indices)
        N = src.shape[0]
        if N == 0:
            return {"loss_mask_temporal_pairwise": self._zero(src.device)}
        pk = tg.pairs()
        row_of_target = torch.full((pk.n_targets,), -1, dtype=torch.int32, device=src.device)
        row_of_target[flat] = torch.arange(N, dtype=torch.int32, device=src.device)
        total, count = ws.temporal_pair_sum(src, row_of_target, pk)
        loss = total / count.to(torch.float32).clamp(min=1.0)
        return {"loss_mask_temporal_pairwise": loss * self._warm()}

    # -- driver ------------------------------------------------------------------------------------------
    def _make_targets(self, targets, device):
        need_sim = "spatial_pairwise" in self.losses or getattr(self.matcher, "cost_pairwise", 0) != 0
        return VideoWeakTargets(targets, device, self.pairwise_color_thresh, need_sim=need_sim)

    def _check(self):
        """The call's one host sync: scipy's ValueErrors for the assignments, IndexError for a pair off the frame."""
        tg = self._tg
        bad_pairs = tg._pairs.bad if tg is not None and tg._pairs is not None else None
        if not self._status and bad_pairs is None:
            return
        dev = bad_pairs.device if bad_pairs is not None else self._status[0].device
        s = torch.stack(self._status).max() if self._status else torch.zeros((), dtype=torch.int32, device=dev)
        b = bad_pairs.to(torch.int32) if bad_pairs is not None else torch.zeros((), dtype=torch.int32, device=dev)
        code = int((s.to(torch.int32) + 16 * b).item())
        if code % 16:
            raise ValueError(ws.LSAP_STATUS.get(code % 16, f"linear_sum_assignment failed ({code % 16})"))
        if code >= 16:
            raise IndexError("temporal_pairs holds a coordinate outside the (H, W) frame")

    def forward(self, outputs, targets):
        losses = super().forward(outputs, targets)
        self._iter_host.step(self._iter)     # after the losses: the first call sees warm-up factor 0
        return losses


class VideoSetCriterionProjSpatPair(VideoSetCriterionProjSpatPairTempPair):
    """Reference: criterion_proj_spatpair.py:74-320 (same constructor; losses without "temporal_pairwise")."""


class VideoSetCriterionProj(VideoSetCriterionProjSpatPairTempPair):
    """Reference: criterion_proj.py:55-280 (five-argument constructor; "labels" and "projection_masks")."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, 3, 2, 0.3, 1, losses)
