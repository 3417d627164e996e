"""Video inference: the eval branch of the reference's ``VideoMaskFormer.forward``
(mask2former_video/video_maskformer_model.py:372-393) and ``inference_video`` (:651-694).

:class:`VideoMaskFormerInference` takes the decoder's *low-resolution* ``pred_masks`` (Q, T, h, w) of a whole video
and never builds the (Q, T, Hp, Wp) fp32 tensor the reference upsamples to (13.5 GB at Q = 100 and 36 frames of
736 x 1280, which is why the reference wraps the call in ``retry_if_cuda_oom``).  The value of a query at an output
pixel of a frame is the chain of ``inference.py``

    F.interpolate((h, w) -> padded (Hp, Wp), bilinear) -> crop to the image (Hc, Wc)
        -> F.interpolate((Hc, Wc) -> (Ho, Wo), bilinear)        [skipped when equal]

evaluated per pixel in fp32 on ``logits.float()`` by ``m2f_infer_video`` (``csrc/video_inference.hip``), which writes
only ``> 0`` of the selected queries: bytes, or with ``packed=True`` one bit per pixel (bit ``x % 32`` of int32 word
``x // 32``, tail bits zero), which cuts the device-to-host copy of the head by 8x.

The class softmax and ``topk(sorted=False)`` over the flattened (Q, K) table stay in torch.  One query may be selected
under several classes; the kernel gets the distinct queries and the entries index its slots.  Scores, labels, slots
and masks travel to the host in one buffer: that copy is the head's only synchronisation.

On CPU tensors the module runs a plain-torch restatement of the same definition (``full_resolution_logits`` per
frame); that is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _native
from .inference import _geometry, _pair, full_resolution_logits
from .rle import _BITS, _encode_device, rle_encode


def pack_mask_bits(masks: torch.Tensor) -> torch.Tensor:
    """(..., W) bool -> (..., ceil(W / 32)) int32, bit x % 32 of word x // 32, tail bits zero."""
    W = masks.shape[-1]
    words = (W + 31) // 32
    m = F.pad(masks.to(torch.int64), (0, words * 32 - W)).view(*masks.shape[:-1], words, 32)
    v = (m << torch.arange(32, dtype=torch.int64, device=masks.device)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def unpack_mask_bits(words: torch.Tensor, width: int) -> torch.Tensor:
    """The inverse of :func:`pack_mask_bits`: (..., ceil(width / 32)) int32 -> (..., width) bool."""
    bits = (words.to(torch.int64)[..., None] >> torch.arange(32, dtype=torch.int64, device=words.device)) & 1
    return bits.flatten(-2)[..., :width].bool()


def _select_slots(Q, S, qidx):
    """The distinct selected queries take the first slots: -> entry -> slot, slot -> query (S,) int32, live slots."""
    mark = torch.zeros(Q, dtype=torch.bool, device=qidx.device).scatter_(0, qidx, True)
    order = torch.sort((~mark).to(torch.uint8), stable=True).indices       # selected queries first
    slot = torch.sort(order).indices.gather(0, qidx)                        # entry -> slot
    return slot, order[:S].to(torch.int32).contiguous(), mark.sum().to(torch.int32).reshape(1)


def _video_masks_hip(mask_pred, qidx, scores, labels, padded_size, geo, packed, keep_bits=False):
    """-> host (scores, labels, slots, masks (S, T, Ho, Wo) bool or (S, T, Ho, words) int32): one copy; and the
    device bit planes (k, T, Ho, words) of the entries with ``keep_bits`` (else None)."""
    masks = mask_pred.detach().contiguous()
    Q, T, h, w = masks.shape
    Hp, Wp = _pair(padded_size)
    Hc, Wc, Ho, Wo = geo
    dev = masks.device
    k = qidx.numel()
    S = min(Q, k)
    slot, sel, n_sel = _select_slots(Q, S, qidx)
    # one int32 buffer: [masks | scores (fp32 bits) | labels | slots]
    row = (Wo + 31) // 32 if packed else Wo
    body = S * T * Ho * row
    words = body if packed else (body + 3) // 4
    buf = torch.empty(words + 3 * k, dtype=torch.int32, device=dev)
    buf[words:words + k] = scores.float().view(torch.int32)
    buf[words + k:words + 2 * k] = labels.to(torch.int32)
    buf[words + 2 * k:] = slot.to(torch.int32)
    _native.call("m2f_infer_video", masks.data_ptr(), _native.dtype_code(masks.dtype, "video inference masks"),
                 sel.data_ptr(), n_sel.data_ptr(), Q, S, T, h, w, Hp, Wp, Hc, Wc, Ho, Wo, int(packed), buf.data_ptr(),
                 _native.stream(masks))
    bits = None
    if keep_bits and packed:
        bits = buf[:body].view(S, T, Ho, row)
    elif keep_bits:                                                         # the byte form holds no planes: a second launch
        bits = torch.empty((S, T, Ho, (Wo + 31) // 32), dtype=torch.int32, device=dev)
        _native.call("m2f_infer_video", masks.data_ptr(), _native.dtype_code(masks.dtype, "video inference masks"),
                     sel.data_ptr(), n_sel.data_ptr(), Q, S, T, h, w, Hp, Wp, Hc, Wc, Ho, Wo, 1, bits.data_ptr(),
                     _native.stream(masks))
    host = buf.cpu()                                                        # the head's one synchronisation
    tail = host[words:]
    if packed:
        out = host[:body].view(S, T, Ho, row)
    else:
        out = host[:words].view(torch.uint8)[:body].view(S, T, Ho, Wo).view(torch.bool)
    if bits is not None:
        bits = bits[slot]                                                   # entries that share a query share a slot
    return tail[:k].view(torch.float32), tail[k:2 * k], tail[2 * k:].tolist(), out, bits


def _video_rle_hip(mask_pred, qidx, scores, labels, padded_size, geo, keep_bits=False):
    """-> host (scores, labels, slots, rles): rles[s] are the T RLE dicts of slot s.  The packed masks stay on the
    device and are encoded there (``csrc/rle.hip``); scores, labels and slots ride with the encoder's first copy.
    With ``keep_bits`` the fifth value is the device bit planes (k, T, Ho, words) of the entries (else None)."""
    masks = mask_pred.detach().contiguous()
    Q, T, h, w = masks.shape
    Hp, Wp = _pair(padded_size)
    Hc, Wc, Ho, Wo = geo
    dev = masks.device
    k = qidx.numel()
    S = min(Q, k)
    slot, sel, n_sel = _select_slots(Q, S, qidx)
    bits = torch.empty((S * T, Ho, (Wo + 31) // 32), dtype=torch.int32, device=dev)
    _native.call("m2f_infer_video", masks.data_ptr(), _native.dtype_code(masks.dtype, "video inference masks"),
                 sel.data_ptr(), n_sel.data_ptr(), Q, S, T, h, w, Hp, Wp, Hc, Wc, Ho, Wo, 1, bits.data_ptr(),
                 _native.stream(masks))
    # slots >= n_sel were not written: they are encoded from slot 0 and never indexed
    live = torch.arange(S, device=dev)
    live = torch.where(live < n_sel, live, torch.zeros_like(live))
    planes = (live[:, None] * T + torch.arange(T, device=dev)).flatten().to(torch.int32)
    extra = torch.cat([scores.float().view(torch.int32), labels.to(torch.int32), slot.to(torch.int32)])
    rles, tail = _encode_device(bits, _BITS, Wo, plane_index=planes, num_masks=S * T, extra=extra)
    tail = tail.to(torch.int32)
    return (tail[:k].view(torch.float32), tail[k:2 * k], tail[2 * k:].tolist(),
            [rles[s * T:(s + 1) * T] for s in range(S)], bits.view(S, T, Ho, -1)[slot] if keep_bits else None)


def _video_masks_cpu(mask_pred, qidx, padded_size, geo, packed):
    """The definition in torch: per frame full_resolution_logits of the selected queries, > 0 (:661-666)."""
    Hc, Wc, Ho, Wo = geo
    frames = [full_resolution_logits(mask_pred[qidx, t], padded_size, (Hc, Wc), (Ho, Wo)) > 0
              for t in range(mask_pred.shape[1])]
    masks = torch.stack(frames, 1)                                          # (k, T, Ho, Wo)
    return pack_mask_bits(masks) if packed else masks


class VideoMaskFormerInference(nn.Module):
    """The eval branch of VideoMaskFormer.forward on the decoder's low-resolution outputs (clip 0, as the
    reference)."""

    def __init__(self, num_classes, test_topk_per_video=10):
        super().__init__()
        if num_classes <= 0 or test_topk_per_video <= 0:
            raise ValueError("num_classes and test_topk_per_video must be positive")
        self.num_classes = int(num_classes)
        self.test_topk_per_video = int(test_topk_per_video)    # the reference's hard-coded 10 (:656)

    @classmethod
    def from_config(cls, cfg):
        return cls(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES)

    @torch.no_grad()
    def forward(self, outputs, padded_size, image_size, output_size=None, packed=False, rle=False, keep_bits=False):
        """outputs: {"pred_logits": (1|B, Q, K+1), "pred_masks": (1|B, Q, T, h, w)}; padded_size (Hp, Wp) of the
        padded frames, image_size (Hc, Wc) without padding, output_size (height, width) (default: the image size).
        Returns the reference's dict: ``image_size`` (the output size), ``pred_scores``, ``pred_labels`` and
        ``pred_masks``, a list of (T, Ho, Wo) bool CPU tensors; with ``packed`` they are (T, Ho, ceil(Wo / 32)) int32
        words (see :func:`unpack_mask_bits`) and the dict also holds ``"packed": True``.  With ``rle`` they are lists
        of T COCO RLE dicts (``bm2f_amd.rle``), encoded on the device from the packed masks, and the dict holds
        ``"rle": True``; entries that share a query share one list.  With ``keep_bits`` the dict also holds
        ``"pred_bits"``, the (k, T, Ho, ceil(Wo / 32)) int32 bit planes of the entries on the device of the inputs
        (what ``bm2f_amd.mask_iou`` and :class:`bm2f_amd.ytvis_eval.YTVISEvaluator` read without a new upload)."""
        if rle and packed:
            raise ValueError("rle=True returns encoded masks; it cannot be combined with packed=True")
        mask_cls, mask_pred = outputs["pred_logits"][0], outputs["pred_masks"][0]
        if mask_pred.dim() != 4:
            raise ValueError("pred_masks must be (B, Q, T, h, w)")
        if mask_cls.shape[-1] != self.num_classes + 1:
            raise ValueError(f"pred_logits has {mask_cls.shape[-1]} columns, expected num_classes + 1")
        geo = _geometry(padded_size, [image_size], [output_size])[0]
        result = {"image_size": (geo[2], geo[3]), "pred_scores": [], "pred_labels": [], "pred_masks": []}
        if packed:
            result["packed"] = True
        if rle:
            result["rle"] = True
        Q, K = mask_pred.shape[0], self.num_classes
        if Q == 0:
            return result
        scores = F.softmax(mask_cls.float(), dim=-1)[:, :-1]
        s, idx = scores.flatten(0, 1).topk(min(self.test_topk_per_video, Q * K), sorted=False)   # :656
        labels, qidx = idx % K, idx // K
        if rle and mask_pred.device.type == "cuda":
            s, labels, slot, masks, bits = _video_rle_hip(mask_pred, qidx, s, labels, padded_size, geo, keep_bits)
        elif mask_pred.device.type == "cuda":
            s, labels, slot, masks, bits = _video_masks_hip(mask_pred, qidx, s, labels, padded_size, geo, packed,
                                                            keep_bits)
        else:
            masks = _video_masks_cpu(mask_pred, qidx, padded_size, geo, packed)
            slot = range(qidx.numel())
            bits = (masks if packed else pack_mask_bits(masks)) if keep_bits else None
            if rle:
                T = masks.shape[1]
                flat = rle_encode(masks)
                masks = [flat[i * T:(i + 1) * T] for i in slot]
        result["pred_scores"] = s.tolist()
        result["pred_labels"] = labels.tolist()
        result["pred_masks"] = [masks[i] for i in slot]
        if keep_bits:
            result["pred_bits"] = bits
        return result
