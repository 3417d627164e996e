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
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import weaksup as ws
from .criterion import _dice_cost, _dist_world, _IterMirror


class _IterCounter(_IterMirror):
    """``_IterMirror`` with a read that does not increment (the criterion steps at the end of forward)."""

    def peek(self, buf):
        if self.value is None:
            self.value = float(buf.item())       # once after construction / load_state_dict
        return self.value


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


class VideoWeakTargets:
    """Per-call target tensors shared by the matcher and every loss of all decoder heads: padded boxes, neighbour
    bits, extents, pairwise denominators and the packed temporal pairs."""

    def __init__(self, targets, device, thresh, need_sim=True):
        self.device = device
        self.cuda = torch.device(device).type == "cuda"
        self.thresh = thresh
        self.B = len(targets)
        self.G = [int(t["labels"].shape[0]) for t in targets]
        self.Gm = max(self.G) if self.G else 0
        self.offsets = np.concatenate([[0], np.cumsum(self.G)]).astype(np.int64).tolist()
        self.labels = [t["labels"].to(device) for t in targets]
        self.box_list = [t["box_masks"].to(device=device, dtype=torch.float32) for t in targets]   # (G, T, H, W)
        self.T, self.H, self.W = (int(v) for v in self.box_list[0].shape[1:]) if self.box_list else (0, 0, 0)
        T, H, W = self.T, self.H, self.W
        self.box_all = torch.cat(self.box_list).reshape(-1, H, W).contiguous() if self.box_list else None  # (Gt*T,..)
        self.bits = self.sim_list = None
        self.shared = True
        if need_sim:
            sims = [t["color_similarities"] for t in targets]
            self.shared = all(s.shape[0] <= 1 or s.stride(0) == 0 for s in sims)
            to_bits = ws.threshold_bits if self.cuda else _bits_torch
            if self.shared:
                # the frame's one map shared across instances -> bits per (clip, frame)
                img = [s[0] if s.shape[0] else s.new_zeros((T, 8, H, W)) for s in sims]
                img = torch.stack([s.to(device=device, dtype=torch.float32) for s in img])       # (B, T, 8, H, W)
                self.bits = to_bits(img.reshape(self.B * T, 8, H, W).contiguous(), thresh)       # (B*T, H, W)
            else:
                self.sim_list = [s.to(device=device, dtype=torch.float32) for s in sims]
                sim_all = torch.cat(self.sim_list).reshape(-1, 8, H, W)
                self.bits = to_bits(sim_all.contiguous(), thresh) if sim_all.shape[0] else None  # (Gt*T, H, W)
        self._targets = targets
        self._padded = self._match_aux = self._pairs = None

    def padded(self):
        """labels (B, Gm) and boxes as frames-as-images (B*T, Gm, H, W)."""
        if self._padded is None:
            B, Gm, T = self.B, self.Gm, self.T
            labels = torch.zeros((B, Gm), dtype=torch.int64, device=self.device)
            box = torch.zeros((B, T, Gm, self.H, self.W), dtype=torch.float32, device=self.device)
            for b in range(B):
                if self.G[b]:
                    labels[b, :self.G[b]] = self.labels[b]
                    box[b, :, :self.G[b]] = self.box_list[b].transpose(0, 1)
            self._padded = (labels, box.view(B * T, Gm, self.H, self.W))
        return self._padded

    def match_aux(self):
        if self._match_aux is None:
            _, box = self.padded()
            B, Gm, T = self.B, self.Gm, self.T
            bx = box.amax(3).view(B, T, Gm, -1).transpose(1, 2).reshape(B, Gm, -1)      # (B, Gm, T*H)
            by = box.amax(2).view(B, T, Gm, -1).transpose(1, 2).reshape(B, Gm, -1)      # (B, Gm, T*W)
            aux = {"box_x": bx, "box_y": by}
            if self.cuda:
                aux["gcount"] = ws.h2d(np.repeat(self.G, T).tolist(), self.device)
                aux["extents"] = ws.box_extents(box)
            if self.shared and self.bits is not None:
                k = torch.arange(8, device=box.device, dtype=torch.uint8)
                tsum = ((self.bits.view(B * T, -1, 1) >> k) & 1).sum(-1, dtype=torch.float32)      # (B*T, HW)
                aux["pair_den"] = (box.view(B * T, Gm, -1) * tsum[:, None]).sum(-1).clamp(min=1.0)  # (B*T, Gm)
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


class VideoHungarianMatcherProjPair(nn.Module):
    """Reference: mask2former_video/modeling/matcher.py:249-393 (same arguments and ``_iter`` buffer);
    ``cost_pairwise = 0`` is ``VideoHungarianMatcherProj`` (:396-501)."""

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
        self.last_status = None

    def _prepare(self, targets, device):
        return VideoWeakTargets(targets, device, self.pairwise_color_thresh, need_sim=self.cost_pairwise != 0)

    @torch.no_grad()
    def cost_matrix(self, outputs, tg: VideoWeakTargets, warm: float) -> torch.Tensor:
        """(B, Q, Gm) fp32 matching cost of every clip (columns >= G_b are padding)."""
        logits, masks = outputs["pred_logits"], outputs["pred_masks"]
        B, Q, T, H, W = masks.shape
        labels, box = tg.padded()
        aux = tg.match_aux()
        Gm = tg.Gm
        prob = logits.float().softmax(-1)
        c_class = -torch.gather(prob, 2, labels[:, None, :].expand(B, Q, Gm))
        # frames as images: the one fp32 cast-and-permute of the masks
        x = torch.empty((B, T, Q, H, W), dtype=torch.float32, device=masks.device)
        x = x.copy_(masks.transpose(1, 2)).view(B * T, Q, H, W)
        want_pair = self.cost_pairwise != 0 and warm != 0
        pair = None
        if tg.cuda and tg.shared and tg.bits is not None:
            # one pass: per-frame pairwise numerators and both axis projections
            num, sx, sy = ws.match_cost(x, tg.bits, box, aux["gcount"], self.pairwise_dilation, aux["extents"])
            pair = (num / aux["pair_den"][:, None, :]).view(B, T, Q, Gm).mean(1)
        else:
            sx, sy = x.amax(3), x.amax(2)
            if want_pair:
                pair = self._pairwise_cost_general(x, tg)
        sx = sx.view(B, T, Q, H).transpose(1, 2).reshape(B, Q, T * H)
        sy = sy.view(B, T, Q, W).transpose(1, 2).reshape(B, Q, T * W)
        c_proj = _dice_cost(sx, aux["box_x"]) + _dice_cost(sy, aux["box_y"])
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
            box = tg.box_list[b]                                                  # (G, T, H, W)
            for t in range(T):
                xf = x[b * T + t].contiguous()
                s = (ws.pairwise_planes(xf, d) if tg.cuda else _pred_similarity(xf, d)).view(Q, -1)
                if tg.shared:
                    k = torch.arange(8, device=x.device, dtype=torch.uint8).view(8, 1, 1)
                    on = ((tg.bits[b * T + t][None] >> k) & 1).float()[None].expand(G, 8, H, W)
                else:
                    on = (tg.sim_list[b][:, t] >= tg.thresh).float()
                tt = (on * box[:, t, None]).reshape(G, -1)
                out[b, :, :G] += (s @ tt.t()) / tt.sum(1)[None].clamp(min=1.0)
        return out / T

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets, prepared: VideoWeakTargets | None = None):
        masks = outputs["pred_masks"]
        tg = prepared or self._prepare(targets, masks.device)
        B, Q = outputs["pred_logits"].shape[:2]
        if tg.Gm == 0:
            e = torch.empty(0, dtype=torch.int64, device=masks.device)
            return [(e, e) for _ in range(B)]
        warm = min(self._iter_host.value / float(self.pairwise_warmup_iters), 1.0)
        C = self.cost_matrix(outputs, tg, warm)
        if tg.cuda:
            match, status = ws.lsap_batched(C, cols=ws.h2d(tg.G, masks.device))
            self.last_status = status
        else:
            from scipy.optimize import linear_sum_assignment
            match = torch.full((B, Q), -1, dtype=torch.int32)
            for b in range(B):
                i, j = linear_sum_assignment(C[b, :, :tg.G[b]].numpy())
                match[b, torch.as_tensor(i, dtype=torch.int64)] = torch.as_tensor(j, dtype=torch.int32)
        return ws.indices_from_match(match, [min(Q, g) for g in tg.G])

    @torch.no_grad()
    def forward(self, outputs, targets, prepared: VideoWeakTargets | None = None):
        self._iter_host.step(self._iter)
        return self.memory_efficient_forward(outputs, targets, prepared)

    def __repr__(self, _repr_indent=4):
        head = "Matcher " + self.__class__.__name__
        body = [f"cost_class: {self.cost_class}", f"cost_projection: {self.cost_projection}",
                f"cost_pairwise: {self.cost_pairwise}", f"pairwise_size: {self.pairwise_size}",
                f"pairwise_dilation: {self.pairwise_dilation}",
                f"pairwise_color_thresh: {self.pairwise_color_thresh}"]
        return "\n".join([head] + [" " * _repr_indent + line for line in body])


class VideoHungarianMatcherProj(VideoHungarianMatcherProjPair):
    """Reference: matcher.py:396-501 (class and projection costs only; no ``_iter`` in its state dict)."""

    def __init__(self, cost_class: float = 1, cost_projection: float = 1):
        assert cost_class != 0 or cost_projection != 0, "all costs cant be 0"
        super().__init__(cost_class, cost_projection, 0, _persistent_iter=False)

    def __repr__(self, _repr_indent=4):
        head = "Matcher " + self.__class__.__name__
        body = [f"cost_class: {self.cost_class}", f"cost_projection: {self.cost_projection}"]
        return "\n".join([head] + [" " * _repr_indent + line for line in body])


class VideoSetCriterionProjSpatPairTempPair(nn.Module):
    """Reference: criterion_proj_spatpair_temppair.py:72-406; ``losses`` is any subset of "labels",
    "projection_masks", "spatial_pairwise", "temporal_pairwise"."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, pairwise_size, pairwise_dilation,
                 pairwise_color_thresh, pairwise_warmup_iters, losses):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.pairwise_size = pairwise_size
        self.pairwise_dilation = pairwise_dilation
        self.pairwise_color_thresh = pairwise_color_thresh
        self.pairwise_warmup_iters = pairwise_warmup_iters
        self.losses = losses
        if pairwise_size != 3:
            raise ValueError("only pairwise_size 3 is implemented")
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.register_buffer("_iter", torch.zeros([1]))
        self._iter_host = _IterCounter(self)
        self.check_matching = True   # one host sync per call (matcher status, pair validity); False skips it
        self._tg = self._tg_key = None
        self._status = []
        self._gathered = {}

    # -- losses ------------------------------------------------------------------------------------------
    def loss_labels(self, outputs, targets, indices, num_masks):
        src_logits = outputs["pred_logits"].float()
        idx = self._get_src_permutation_idx(indices)
        target_classes_o = torch.cat([t["labels"].to(src_logits.device)[J] for t, (_, J) in zip(targets, indices)])
        target_classes = torch.full(src_logits.shape[:2], self.num_classes, dtype=torch.int64,
                                    device=src_logits.device)
        target_classes[idx] = target_classes_o
        return {"loss_ce": F.cross_entropy(src_logits.transpose(1, 2), target_classes, self.empty_weight)}

    def _matched(self, outputs, targets, indices):
        """Matched masks (N, T, H, W) fp32 and flat target rows, gathered once per head for all mask losses."""
        tg = self._targets(targets, outputs["pred_masks"].device)
        key = (id(outputs["pred_masks"]), id(indices))
        hit = self._gathered.get(key)
        if hit is not None and hit[0] is outputs["pred_masks"] and hit[1] is indices:
            return tg, hit[2], hit[3]
        src = outputs["pred_masks"][self._get_src_permutation_idx(indices)].float().contiguous()
        flat = torch.cat([j + tg.offsets[b] for b, (_, j) in enumerate(indices)])
        self._gathered[key] = (outputs["pred_masks"], indices, src, flat)
        return tg, src, flat

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
            k = torch.arange(8, dtype=torch.uint8).view(1, 8, 1, 1)
            on = ((tg.bits[t_row][:, None] >> k) & 1).float() * tg.box_all[box_row][:, None]
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

    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        return batch_idx, src_idx

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        tgt_idx = torch.cat([tgt for (_, tgt) in indices])
        return batch_idx, tgt_idx

    def get_loss(self, loss, outputs, targets, indices, num_masks):
        loss_map = {"labels": self.loss_labels, "projection_masks": self.loss_projection_masks,
                    "spatial_pairwise": self.loss_spatial_pairwise,
                    "temporal_pairwise": self.loss_temporal_pairwise}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](outputs, targets, indices, num_masks)

    # -- driver ------------------------------------------------------------------------------------------
    def _targets(self, targets, device):
        # built once per forward() for all heads; a direct get_loss() call outside forward builds its own
        if self._tg is None or self._tg_key is not targets:
            need_sim = "spatial_pairwise" in self.losses or getattr(self.matcher, "cost_pairwise", 0) != 0
            self._tg = VideoWeakTargets(targets, device, self.pairwise_color_thresh, need_sim=need_sim)
            self._tg_key = targets
        return self._tg

    def _match(self, outputs, targets):
        if isinstance(self.matcher, VideoHungarianMatcherProjPair):
            self.matcher.last_status = None
            idx = self.matcher(outputs, targets, prepared=self._targets(targets, outputs["pred_masks"].device))
            if self.matcher.last_status is not None:
                self._status.append(self.matcher.last_status)
            return idx
        return self.matcher(outputs, targets)

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
        self._tg = self._tg_key = None
        self._status = []
        self._gathered = {}
        try:
            outputs_without_aux = {k: v for k, v in outputs.items() if k != "aux_outputs"}
            indices = self._match(outputs_without_aux, targets)
            dev = next(iter(outputs.values())).device
            n = sum(len(t["labels"]) for t in targets)
            world = _dist_world()
            if world:
                nm = torch.as_tensor([n], dtype=torch.float, device=dev)
                torch.distributed.all_reduce(nm)
                num_masks = torch.clamp(nm / world, min=1)[0]      # stays on the device (no .item())
            else:
                num_masks = max(float(np.float32(n)), 1.0)
            losses = {}
            for loss in self.losses:
                losses.update(self.get_loss(loss, outputs, targets, indices, num_masks))
            for i, aux_outputs in enumerate(outputs.get("aux_outputs", [])):
                indices = self._match(aux_outputs, targets)
                for loss in self.losses:
                    l_dict = self.get_loss(loss, aux_outputs, targets, indices, num_masks)
                    losses.update({k + f"_{i}": v for k, v in l_dict.items()})
            if self.check_matching:
                self._check()
            self._iter_host.step(self._iter)
            return losses
        finally:
            self._tg = self._tg_key = None
            self._status = []
            self._gathered = {}

    def __repr__(self):
        head = "Criterion " + self.__class__.__name__
        body = [f"matcher: {self.matcher.__repr__(_repr_indent=8)}", f"losses: {self.losses}",
                f"weight_dict: {self.weight_dict}", f"num_classes: {self.num_classes}", f"eos_coef: {self.eos_coef}"]
        return "\n".join([head] + [" " * 4 + line for line in body])


class VideoSetCriterionProjSpatPair(VideoSetCriterionProjSpatPairTempPair):
    """Reference: criterion_proj_spatpair.py:74-320 (same constructor; losses without "temporal_pairwise")."""


class VideoSetCriterionProj(VideoSetCriterionProjSpatPairTempPair):
    """Reference: criterion_proj.py:55-280 (five-argument constructor; "labels" and "projection_masks")."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, 3, 2, 0.3, 1, losses)
