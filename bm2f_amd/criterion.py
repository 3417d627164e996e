"""Box-supervised Hungarian matcher and set criterion on the GPU.

Drop-ins for the reference's ``HungarianMatcherProjPair`` (mask2former/modeling/matcher.py:213-337) and
``SetCriterionProjPair`` (mask2former/modeling/criterion.py:184-442): same constructor arguments, buffers
(``_iter``, ``empty_weight``: checkpoints load), ``forward(outputs, targets)`` contracts and loss keys
(``loss_ce``, ``loss_mask_projection``, ``loss_pairwise`` and the ``_i`` aux copies).

What changes is where the work runs.  The reference loops over images, builds each (Q, G) cost on the
device, copies it to the host and calls scipy per image per decoder head (matcher.py:309-311: 10 x batch
host round trips per step), and reads ``_iter`` / ``num_masks`` back with ``.item()``.  Here

* the three costs are computed for the whole batch at once: class cost by one gather; projection dice
  by batched GEMMs over the row / column maxima; the pairwise-affinity cost by one kernel pass over all
  B*Q masks (``m2f_pairwise_rows`` mode 0: sum_k bit_k s_k per pixel, s = -log P(same label) of the 8
  dilated neighbours, bit_k = colour similarity >= thresh) followed by a (Q x HW) x (HW x G) GEMM against
  the box masks -- exact because the reference's per-target similarity is the image's one map repeated
  G times (maskformer_model.py:498-500); a per-target similarity falls back to the general form
  s (Q, 8HW) x T (8HW, G);
* all B assignments are solved in one launch of the GPU LSAP (``m2f_lsap_batched``: scipy's algorithm
  and tie rule in fp64) and turned into index tensors without a host sync;
* the pairwise loss is one fused forward / backward kernel pair over the matched masks (no (N, 8, H, W)
  intermediates);
* ``_iter`` is mirrored on the host, ``num_masks`` stays a device scalar under torch.distributed, and
  LSAP failures (NaN / -inf / infeasible costs, which scipy raises for) are checked once per criterion call
  (``check_matching = False`` on the criterion skips that one sync).

Matched indices are returned as int64 tensors on the masks' device (the reference returns CPU tensors;
both index the same way).

The matcher and the targets are the video ones (video_criterion.py) on clips of one frame; the driver is
set_criterion.py.  What is the image criterion's own is below: its two mask losses (HIP tensors only) and the
``_iter`` step before matching.
"""
from __future__ import annotations

import torch

from . import weaksup as ws
from .set_criterion import _IterMirror, _SetCriterion
from .video_criterion import VideoHungarianMatcherProjPair, VideoWeakTargets


class WeakTargets(VideoWeakTargets):
    """Per-call device-side target tensors shared by the matcher and every loss of all decoder heads: the video
    targets for clips of one frame (``box_masks`` (G, H, W), ``images_color_similarity`` (G, 8, H, W))."""

    _sim_key = "images_color_similarity"


class HungarianMatcherProjPair(VideoHungarianMatcherProjPair):
    """Reference: mask2former/modeling/matcher.py:213-337 (same arguments and ``_iter`` buffer).  The video
    matcher on one-frame clips: one frame's axis maxima are the image's, and the mean over one frame of
    num / pair_den is num / pair_den."""

    _repr_fields = ("cost_class", "cost_projection", "cost_pairwise")

    def __init__(self, cost_class: float = 1, cost_projection: float = 1, cost_pairwise: float = 1,
                 pairwise_size: int = 3, pairwise_dilation: int = 2, pairwise_color_thresh: float = 0.3,
                 pairwise_warmup_iters: int = 10000, point_sample: bool = False, num_points: int = 12544):
        super().__init__(cost_class, cost_projection, cost_pairwise, pairwise_size, pairwise_dilation,
                         pairwise_color_thresh, pairwise_warmup_iters)
        self.point_sample = point_sample
        self.num_points = num_points

    def _prepare(self, targets, device):
        return WeakTargets(targets, device, self.pairwise_color_thresh)


class SetCriterionProjPair(_SetCriterion):
    """Reference: mask2former/modeling/criterion.py:184-442 (losses "labels", "projection_masks",
    "pairwise"; point sampling is not used by this criterion in the reference either)."""

    _matcher_class = HungarianMatcherProjPair
    _loss_table = {"labels": "loss_labels", "projection_masks": "loss_projection_masks",
                   "pairwise": "loss_pairwise"}

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, pairwise_size, pairwise_dilation,
                 pairwise_color_thresh, pairwise_warmup_iters, losses, point_sample, num_points, oversample_ratio,
                 importance_sample_ratio):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, losses)
        self.pairwise_size = pairwise_size
        self.pairwise_dilation = pairwise_dilation
        self.pairwise_color_thresh = pairwise_color_thresh
        self.pairwise_warmup_iters = pairwise_warmup_iters
        self.point_sample = point_sample
        if point_sample:
            self.num_points = num_points
            self.oversample_ratio = oversample_ratio
            self.importance_sample_ratio = importance_sample_ratio
        if pairwise_size != 3:
            raise ValueError("only pairwise_size 3 is implemented")
        self.register_buffer("_iter", torch.zeros([1]))
        self._iter_host = _IterMirror(self)

    # -- losses (HIP tensors only) -------------------------------------------------------------------

    def loss_projection_masks(self, outputs, targets, indices, num_masks):
        tg, src, flat = self._matched(outputs, targets, indices)
        box = tg.box_all[flat]
        x = src.max(dim=2)[0].sigmoid()          # projection on the H axis (max over W), criterion.py:353
        y = src.max(dim=1)[0].sigmoid()
        with torch.no_grad():
            bx = box.max(dim=2)[0]
            by = box.max(dim=1)[0]

        def dice(p, t):
            inter = (p * t).sum(dim=1)
            union = (p ** 2.0).sum(dim=1) + (t ** 2.0).sum(dim=1) + 1e-3
            return 1. - (2 * inter / union)

        return {"loss_mask_projection": (dice(x, bx) + dice(y, by)).sum() / num_masks}

    def loss_pairwise(self, outputs, targets, indices, num_masks):
        tg, src, flat = self._matched(outputs, targets, indices)
        box_row = flat.to(torch.int32)
        if tg.shared:
            t_row = self._get_src_permutation_idx(indices)[0].to(torch.int32)
        else:
            t_row = box_row
        bits = tg.bits if tg.bits is not None else torch.zeros((1, tg.H, tg.W), dtype=torch.uint8,
                                                                 device=src.device)
        num, den = ws.pairwise_sums(src, bits, t_row.contiguous(), tg.box_all, box_row.contiguous(),
                                    self.pairwise_dilation)
        warm = min(self._iter_host.value / float(self.pairwise_warmup_iters), 1.0)
        return {"loss_pairwise": num.sum() / den.sum().clamp(min=1.0) / num_masks * warm}

    # -- driver --------------------------------------------------------------------------------------
    def _make_targets(self, targets, device):
        return WeakTargets(targets, device, self.pairwise_color_thresh)

    def forward(self, outputs, targets):
        self._iter_host.step(self._iter)     # before matching: the first call sees warm-up factor 1 / warmup
        return super().forward(outputs, targets)
