"""What the three matcher / set-criterion families share: box-supervised image (criterion.py), box-supervised
video (video_criterion.py) and mask-supervised image and video (mask_criterion.py).

The families differ in their targets, matching costs and mask losses.  The driver around those is one: targets
prepared once per ``forward`` for all decoder heads, one batched assignment per head (``m2f_lsap_batched`` on a HIP
tensor, scipy on a CPU tensor), ``num_masks`` as a device scalar under torch.distributed, the class loss, and one
host sync per criterion call for the matcher status (``check_matching = False`` skips it).  On a HIP tensor a kernel
error raises; nothing falls back to torch.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from . import weaksup as ws


def _dist_world():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_world_size()
    return 0


def _num_masks(targets, device):
    """Targets per step averaged over the ranks, at least 1: a device scalar after all_reduce, else a host float."""
    n = sum(len(t["labels"]) for t in targets)
    world = _dist_world()
    if world:
        nm = torch.as_tensor([n], dtype=torch.float, device=device)
        torch.distributed.all_reduce(nm)
        return torch.clamp(nm / world, min=1)[0]      # stays on the device (no .item())
    return max(float(np.float32(n)), 1.0)


class _IterMirror:
    """Host copy of a float32 ``_iter`` buffer so the warm-up factor needs no ``.item()`` per call."""

    def __init__(self, module):
        self.value = None
        module._register_load_state_dict_pre_hook(self._invalidate)

    def _invalidate(self, *args, **kwargs):
        self.value = None

    def peek(self, buf):
        if self.value is None:
            self.value = float(buf.item())       # once after construction / load_state_dict
        return self.value

    def step(self, buf):
        buf += 1
        if self.value is None:
            return self.peek(buf)
        self.value = float(np.float32(self.value) + np.float32(1.0))
        return self.value


def _dice_cost(src, tgt):
    """Batched batch_dice_loss (matcher.py:103-121): src (B, Q, L) logits, tgt (B, G, L)."""
    s = src.sigmoid()
    num = 2 * torch.bmm(s, tgt.transpose(1, 2))
    den = s.sum(-1)[:, :, None] + tgt.sum(-1)[:, None, :]
    return 1 - (num + 1) / (den + 1)


def _class_cost(logits, labels):
    """-softmax(logits)[b, q, labels[b, g]]: logits (B, Q, K+1), padded labels (B, Gm) -> (B, Q, Gm)."""
    B, Q = logits.shape[:2]
    return -torch.gather(logits.float().softmax(-1), 2, labels[:, None, :].expand(B, Q, labels.shape[1]))


def _bit_planes(bits):
    """(N, H, W) uint8 neighbour bits -> (N, 8, H, W) uint8, plane k = bit k."""
    k = torch.arange(8, device=bits.device, dtype=torch.uint8).view(8, 1, 1)
    return (bits[:, None] >> k) & 1


class _Targets:
    """What every family's per-call target tensors start from: the counts, flat row offsets and labels."""

    def __init__(self, targets, device):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.B = len(targets)
        self.G = [int(t["labels"].shape[0]) for t in targets]
        self.Gm = max(self.G) if self.G else 0
        self.offsets = np.concatenate([[0], np.cumsum(self.G)]).astype(np.int64).tolist()
        self.labels = [t["labels"].to(device) for t in targets]
        self._targets = targets
        self._labels_padded = None

    def labels_padded(self):
        """(B, Gm) int64, zero beyond an image's G."""
        if self._labels_padded is None:
            self._labels_padded = pad_sequence([l.long() for l in self.labels], batch_first=True)
        return self._labels_padded


class _Matcher(nn.Module):
    """A matcher is its ``cost_matrix(outputs, tg, *args) -> (B, Q, Gm)``; the assignment is shared."""

    last_status = None       # (B,) LSAP status of the last assignment on a HIP tensor; the criterion checks it

    def _assign(self, outputs, tg, *cost_args):
        """Per image / clip (query idx, target idx) int64 on the masks' device; no host sync on a HIP tensor."""
        B, Q = outputs["pred_logits"].shape[:2]
        if tg.Gm == 0:
            e = torch.empty(0, dtype=torch.int64, device=outputs["pred_masks"].device)
            return [(e, e) for _ in range(B)]
        C = self.cost_matrix(outputs, tg, *cost_args)
        if C.is_cuda:
            match, status = ws.lsap_batched(C, cols=ws.h2d(tg.G, C.device))
            self.last_status = status
        else:
            from scipy.optimize import linear_sum_assignment
            match = torch.full((B, Q), -1, dtype=torch.int32)
            for b in range(B):
                i, j = linear_sum_assignment(C[b, :, :tg.G[b]].numpy())
                match[b, torch.as_tensor(i, dtype=torch.int64)] = torch.as_tensor(j, dtype=torch.int32)
        return ws.indices_from_match(match, [min(Q, g) for g in tg.G])

    def _repr(self, fields, indent):
        head = "Matcher " + self.__class__.__name__
        return "\n".join([head] + [" " * indent + f"{f}: {getattr(self, f)}" for f in fields])


class _SetCriterion(nn.Module):
    """The driver of every criterion.  A family sets ``_matcher_class`` (the matcher that takes prepared targets),
    ``_loss_table`` (loss name -> method name) and ``_make_targets``; it may extend ``_matcher_kwargs``,
    ``_check`` and ``_repr_body``."""

    _matcher_class = ()
    _loss_table = {"labels": "loss_labels"}

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.check_matching = True   # one host sync per call for scipy's ValueErrors; False skips it
        self._reset()

    def _reset(self):
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
        """Matched masks (N, [T,] H, W) fp32 and flat target rows, gathered once per head for all mask losses of
        the box-supervised criteria (one IndexBackward, so one full-size gradient buffer per head)."""
        tg = self._targets(targets, outputs["pred_masks"].device)
        key = (id(outputs["pred_masks"]), id(indices))
        hit = self._gathered.get(key)
        if hit is not None and hit[0] is outputs["pred_masks"] and hit[1] is indices:
            return tg, hit[2], hit[3]
        src = outputs["pred_masks"][self._get_src_permutation_idx(indices)].float().contiguous()
        flat = torch.cat([j + tg.offsets[b] for b, (_, j) in enumerate(indices)])                # target rows
        self._gathered[key] = (outputs["pred_masks"], indices, src, flat)
        return tg, src, flat

    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        return batch_idx, src_idx

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        tgt_idx = torch.cat([tgt for (_, tgt) in indices])
        return batch_idx, tgt_idx

    def get_loss(self, loss, outputs, targets, indices, num_masks):
        assert loss in self._loss_table, f"do you really want to compute {loss} loss?"
        return getattr(self, self._loss_table[loss])(outputs, targets, indices, num_masks)

    # -- driver ------------------------------------------------------------------------------------------
    def _make_targets(self, targets, device):
        raise NotImplementedError

    def _targets(self, targets, device):
        # built once per forward() for all heads; a direct get_loss() call outside forward builds its own
        if self._tg is None or self._tg_key is not targets:
            self._tg = self._make_targets(targets, device)
            self._tg_key = targets
        return self._tg

    def _matcher_kwargs(self):
        return {}

    def _match(self, outputs, targets):
        m = self.matcher
        if not isinstance(m, self._matcher_class):
            return m(outputs, targets)
        m.last_status = None         # a call that returns early (no targets) must not report the previous one's
        idx = m(outputs, targets, prepared=self._targets(targets, outputs["pred_masks"].device),
                **self._matcher_kwargs())
        if m.last_status is not None:
            self._status.append(m.last_status)
        return idx

    def _check(self):
        """The call's one host sync: scipy's ValueErrors for the assignments."""
        if self._status:
            ws.raise_on_lsap_status(torch.stack(self._status))

    def forward(self, outputs, targets):
        self._reset()
        try:
            outputs_without_aux = {k: v for k, v in outputs.items() if k != "aux_outputs"}
            indices = self._match(outputs_without_aux, targets)
            num_masks = _num_masks(targets, next(iter(outputs.values())).device)
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
            return losses
        finally:
            self._reset()

    def _repr_body(self):
        return [f"matcher: {self.matcher.__repr__(_repr_indent=8)}", f"losses: {self.losses}",
                f"weight_dict: {self.weight_dict}", f"num_classes: {self.num_classes}", f"eos_coef: {self.eos_coef}"]

    def __repr__(self):
        head = "Criterion " + self.__class__.__name__
        return "\n".join([head] + [" " * 4 + line for line in self._repr_body()])
