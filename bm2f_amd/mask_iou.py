"""Mask IoU on one-bit-per-pixel planes: what the reference's video evaluator gets from ``pycocotools.mask.merge``
and ``area`` once per detection, ground truth and frame (``computeIoU``,
mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:176-222).

The planes are those of ``pack_mask_bits`` and of the video head's ``packed=True`` / ``keep_bits=True`` outputs:
(H, ceil(W / 32)) int32, bit ``x % 32`` of word ``x // 32``, tail bits zero.

:func:`rle_to_bits`       COCO RLE dicts (``bm2f_amd.rle``) -> planes.  The strings are parsed on the host with
                          vectorised numpy into cumulative run ends, checked there, and expanded on the device by
                          ``m2f_rle_decode_bits`` (``csrc/mask_iou.hip``).
:func:`mask_pair_counts`  planes of Da and Db instance sequences -> intersection (Da, Db) and per-frame areas, summed
                          with popcounts by ``m2f_bits_pair_counts``; only those integers reach the host, in one copy.
:func:`mask_iou`          counts -> IoU in float64.

On CPU tensors a numpy restatement of the same definitions runs; that is not a fallback: on a HIP tensor a kernel
error raises ``NativeError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native

_MAX_MASKS = 65535                     # m2f_rle_decode_bits: masks per launch
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def pair_tiles():
    """(TA, TB, chunk_words) of ``m2f_bits_pair_counts``: the instance tile and the word positions of a workgroup."""
    ta, tb, cw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.call("m2f_bits_pair_tiles", ctypes.byref(ta), ctypes.byref(tb), ctypes.byref(cw))
    return ta.value, tb.value, cw.value


# -------------------------------------------------------------------------------------------------------------------
# RLE -> cumulative run ends (host, vectorised)
# -------------------------------------------------------------------------------------------------------------------
def _seg_cumsum(values, lengths):
    """Inclusive cumulative sums of ``values`` restarted at every segment (``lengths`` sums to values.size)."""
    cs = np.cumsum(values, dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lengths)))[:-1]
    base = np.concatenate(([0], cs))[starts]
    return cs - np.repeat(base, lengths)


def _parse_strings(strings):
    """Compressed counts of many masks -> (counts (n,) int64, counts per mask (len(strings),))."""
    raw = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strings]
    nchar = np.array([len(r) for r in raw], dtype=np.int64)
    c = np.frombuffer(b"".join(raw), dtype=np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64), np.zeros(len(raw), np.int64)
    if (c < 0).any() or (c > 63).any():
        raise ValueError("counts hold characters outside the RLE alphabet")
    last = (c & 0x20) == 0                                           # the last character of a value
    str_end = np.cumsum(nchar)[nchar > 0] - 1
    if not last[str_end].all():
        raise ValueError("counts end inside a value")
    first = np.concatenate(([True], last[:-1]))
    start = np.flatnonzero(first)
    k = np.arange(c.size) - np.repeat(start, np.diff(np.concatenate((start, [c.size]))))
    if (k > 7).any():
        raise ValueError("a count takes more than 8 characters")
    x = np.add.reduceat((c & 0x1f) << (5 * k), start)
    end = np.flatnonzero(last)
    x = np.where((c[end] & 0x10) != 0, x | (np.int64(-1) << (5 * (k[end] + 1))), x)
    # values per mask, then counts[i] = x[i] + counts[i - 2] for i > 2: sums along the odd and the even (>= 2) chains
    mask_of_char = np.repeat(np.arange(len(raw)), nchar)
    n = np.bincount(mask_of_char[end], minlength=len(raw)).astype(np.int64)
    idx = np.arange(x.size) - np.repeat(np.concatenate(([0], np.cumsum(n)))[:-1], n)
    counts = x.copy()
    odd = idx % 2 == 1
    even = (idx % 2 == 0) & (idx >= 2)
    counts[odd] = _seg_cumsum(x[odd], n // 2)
    counts[even] = _seg_cumsum(x[even], np.maximum((n + 1) // 2 - 1, 0))
    return counts, n


def _run_ends(rles, size=None):
    """-> (positions (n,) int32 cumulative run ends, offsets (M + 1,) int64, H, W); every check of rle_to_bits."""
    rles = list(rles)
    for r in rles:
        if r is not None:
            if size is None:
                size = r["size"]
            if [int(v) for v in r["size"]] != [int(v) for v in size]:
                raise ValueError(f"masks of different sizes: {list(r['size'])} and {list(size)}")
    if size is None:
        raise ValueError("no mask gives the size; pass size=(H, W)")
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"{H} x {W} pixels: sizes must be positive and fit a 32-bit count")
    M = len(rles)
    n = np.zeros(M, dtype=np.int64)
    is_str = np.array([r is not None and isinstance(r["counts"], (str, bytes)) for r in rles], dtype=bool)
    is_list = np.array([r is not None and not isinstance(r["counts"], (str, bytes)) for r in rles], dtype=bool)
    parts = {}
    if is_str.any():
        c, k = _parse_strings([rles[i]["counts"] for i in np.flatnonzero(is_str)])
        n[is_str] = k
        parts["str"] = c
    lists = [np.asarray(rles[i]["counts"], dtype=np.int64).reshape(-1) for i in np.flatnonzero(is_list)]
    if lists:
        n[is_list] = [a.size for a in lists]
        parts["list"] = np.concatenate(lists)
    offsets = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    counts = np.zeros(int(offsets[-1]), dtype=np.int64)
    owner = np.repeat(np.arange(M), n)
    if "str" in parts:
        counts[is_str[owner]] = parts["str"]
    if "list" in parts:
        counts[is_list[owner]] = parts["list"]
    if (counts < 0).any():
        raise ValueError("negative counts")
    ends = _seg_cumsum(counts, n)
    present = is_str | is_list
    if (n[present] == 0).any() or (ends[offsets[1:][present] - 1] != H * W).any():
        raise ValueError("counts do not add up to the mask size")
    return ends.astype(np.int32), offsets, H, W


def _pack_rows(bits):
    """(..., W) bool numpy -> (..., ceil(W / 32)) int32 words, bit x % 32 of word x // 32."""
    W = bits.shape[-1]
    words = (W + 31) // 32
    pad = np.zeros(bits.shape[:-1] + (words * 32,), dtype=np.uint8)
    pad[..., :W] = bits
    return np.packbits(pad, axis=-1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def _decode_host(positions, offsets, H, W):
    M = offsets.size - 1
    out = np.zeros((M, H, (W + 31) // 32), dtype=np.int32)
    for m in range(M):
        t = positions[offsets[m]:offsets[m + 1]]
        if t.size:
            flips = np.bincount(t[t < H * W], minlength=H * W)       # pixel p is set when an odd number of ends <= p
            out[m] = _pack_rows((np.cumsum(flips) & 1).astype(bool).reshape(W, H).T)
    return out


def rle_to_bits(rles, device=None, size=None) -> torch.Tensor:
    """rles: RLE dicts ``{"size": [H, W], "counts": ...}`` of one size; ``counts`` is a compressed string or bytes, or
    the uncompressed list of run lengths (as in YTVIS ground truth); an entry may be ``None`` (a missing frame: a zero
    plane; ``size`` gives (H, W) when every entry is None).  -> (M, H, ceil(W / 32)) int32 on ``device``.

    Raises ValueError, before any launch, when a count is negative, the counts of a mask do not sum to H * W, a
    string is malformed or the sizes differ."""
    device = torch.device("cpu" if device is None else device)
    rles = list(rles)
    if not rles:
        if size is None:
            raise ValueError("no mask gives the size; pass size=(H, W)")
        return torch.zeros((0, int(size[0]), (int(size[1]) + 31) // 32), dtype=torch.int32, device=device)
    positions, offsets, H, W = _run_ends(rles, size)
    M = len(rles)
    if device.type != "cuda":
        return torch.from_numpy(_decode_host(positions, offsets, H, W)).to(device)
    words = (W + 31) // 32
    # one upload: [offsets as int32 pairs | positions]
    host = np.concatenate((offsets.view(np.int32), positions))
    buf = torch.from_numpy(host).to(device)
    off = buf[:2 * (M + 1)].view(torch.int64)
    pos = buf[2 * (M + 1):]
    out = torch.empty((M, H, words), dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        for m0 in range(0, M, _MAX_MASKS):
            m1 = min(M, m0 + _MAX_MASKS)
            _native.call("m2f_rle_decode_bits", pos.data_ptr() if pos.numel() else None, pos.numel(),
                         off[m0:].data_ptr(), m1 - m0, H, W, out[m0:].data_ptr(), st)
    return out


# -------------------------------------------------------------------------------------------------------------------
# pair counts
# -------------------------------------------------------------------------------------------------------------------
def _instances(t, n):
    """(D, T, H, words) -> the tensor with every instance contiguous (itself where the strides allow it) and the
    instance stride in words; ``n`` is the number of words of an instance."""
    if not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < n):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else n)


def _popcount(words):
    return _POP8[np.ascontiguousarray(words).view(np.uint8)].reshape(*words.shape, 4).sum(-1)


def _pair_counts_host(a, b, width):
    keep = np.full(a.shape[-1], -1, dtype=np.int32)
    if width % 32:
        keep[-1] = (1 << (width % 32)) - 1
    a, b = a & keep, b & keep
    inter = np.zeros((a.shape[0], b.shape[0]), dtype=np.int64)
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            inter[i, j] = _popcount(a[i] & b[j]).sum()
    return inter, _popcount(a).sum((2, 3)), _popcount(b).sum((2, 3))


def mask_pair_counts(a_bits, b_bits, width):
    """a_bits (Da, T, H, words), b_bits (Db, T, H, words) int32 planes of ``width`` columns (``words`` =
    ceil(width / 32); set tail bits are ignored) -> host int64 arrays ``inter`` (Da, Db), the number of pixels set
    in both over all frames, ``area_a`` (Da, T) and ``area_b`` (Db, T).  On HIP tensors one launch of
    ``m2f_bits_pair_counts`` and one device-to-host copy.  With ``Da == 0`` or ``Db == 0`` ``inter`` and the areas of
    the empty side are empty and nothing is launched for them; the areas of the other side, when it has instances,
    are still counted."""
    for t in (a_bits, b_bits):
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.int32:
            raise ValueError("planes must be (D, T, H, words) int32 tensors")
    Da, T, H, words = a_bits.shape
    Db = b_bits.shape[0]
    W = int(width)
    if tuple(b_bits.shape[1:]) != (T, H, words) or W <= 0 or words != (W + 31) // 32:
        raise ValueError("a and b must share (T, H, ceil(width / 32))")
    if a_bits.device != b_bits.device:
        raise ValueError("a and b must be on one device")
    if T == 0 or H == 0:
        raise ValueError("empty planes")
    if Da == 0 or Db == 0:
        inter, none = np.zeros((Da, Db), np.int64), np.zeros((0, T), np.int64)
        if Da == Db == 0:
            return inter, none, none
        one = a_bits if Da else b_bits                                # the other side still has areas to count
        area = mask_pair_counts(one, one[:1], W)[1]
        return (inter, area, none) if Da else (inter, none, area)
    if a_bits.device.type != "cuda":
        return _pair_counts_host(a_bits.detach().numpy(), b_bits.detach().numpy(), W)
    dev = a_bits.device
    a, sa = _instances(a_bits.detach(), T * H * words)
    b, sb = _instances(b_bits.detach(), T * H * words)
    nbytes = ctypes.c_int64()
    _native.call("m2f_bits_pair_workspace", Da, Db, T, H, W, ctypes.byref(nbytes))
    work = torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=dev)
    out = torch.empty(Da * Db + (Da + Db) * T, dtype=torch.int64, device=dev)
    n0, n1 = Da * Db, Da * Db + Da * T
    with torch.cuda.device(dev):
        _native.call("m2f_bits_pair_counts", a.data_ptr(), Da, sa, b.data_ptr(), Db, sb, T, H, W, out.data_ptr(),
                     out[n0:].data_ptr(), out[n1:].data_ptr(), work.data_ptr(), work.numel() * 4,
                     torch.cuda.current_stream(dev).cuda_stream)
    host = out.cpu().numpy()                                          # the one copy
    return host[:n0].reshape(Da, Db), host[n0:n1].reshape(Da, T), host[n1:].reshape(Db, T)


def mask_iou(inter, area_a, area_b, iscrowd=None) -> np.ndarray:
    """inter (Da, Db), area_a (Da,) and area_b (Db,) counts (per-frame areas (D, T) are summed over T) -> float64
    (Da, Db): ``i / u`` with ``u = area_a + area_b - i``, ``0.0`` where ``u == 0`` (``iou_seq``, ytvoseval.py:203-217).
    Where ``iscrowd[j]`` is true ``u = area_a`` (the pycocotools rule for crowd regions; the video evaluator does not
    use it)."""
    i = np.asarray(inter, dtype=np.float64)
    a = np.asarray(area_a, dtype=np.float64)
    b = np.asarray(area_b, dtype=np.float64)
    a = a.reshape(a.shape[0], -1).sum(1) if a.ndim else a
    b = b.reshape(b.shape[0], -1).sum(1) if b.ndim else b
    u = a[:, None] + b[None, :] - i
    if iscrowd is not None:
        crowd = np.asarray(iscrowd, dtype=bool)
        u = np.where(crowd[None, :], np.broadcast_to(a[:, None], u.shape), u)
    out = np.zeros_like(u)
    np.divide(i, u, out=out, where=u > 0)
    return out
