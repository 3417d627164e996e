"""COCO run-length encoding (RLE) of binary masks: the form the reference's evaluators consume
(``pycocotools.mask.encode`` in mask2former_video/data_video/ytvis_eval.py:256-293), restated here.

The format
    A mask (H, W) is read column-major: pixel ``p = x * H + y``.  ``counts`` are the lengths of alternating runs,
    starting with a run of zeros (``counts[0] == 0`` when pixel 0 is set; an all-zero mask is ``[H * W]``).  With
    ``t_0 < ... < t_{k-1}`` the positions where ``pixel(p) != pixel(p - 1)`` and ``pixel(-1) = 0``,
    ``counts = [t_0, t_1 - t_0, ..., H * W - t_{k-1}]``.  The string holds, per run ``i``, the value
    ``x = counts[i] - (counts[i - 2] if i > 2 else 0)`` in 5-bit groups, low group first: ``c = x & 0x1f``,
    ``x >>= 5`` (arithmetic), ``more = (x != -1) if c & 0x10 else (x != 0)``, ``c |= 0x20`` if more, ``chr(c + 48)``.
    An RLE is ``{"size": [H, W], "counts": str}``.

:func:`rle_encode` on a HIP tensor runs the four kernels of ``csrc/rle.hip`` (``m2f_rle_*`` in ``include/bm2f.h``)
with two ``torch.cumsum`` scans between them; the host receives the per-mask run totals (to size the buffers) and
then the encoded bytes with their offsets, never a mask.  On a CPU tensor it runs a vectorised numpy restatement of
the definition; that is not a fallback: on a HIP tensor a kernel error raises ``NativeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native

_BITS, _BYTES = 0, 1
_GROUP_LIMITS = (1 << 4, 1 << 9, 1 << 14, 1 << 19, 1 << 24, 1 << 29)   # a count >= limit k needs > k + 1 chars


# -------------------------------------------------------------------------------------------------------------------
# strings
# -------------------------------------------------------------------------------------------------------------------
def _delta_chars(delta):
    """delta (n,) int64 -> chars (n, 7) uint8 and live (n, 7) bool: the characters of every value, in order."""
    x = np.asarray(delta, dtype=np.int64).copy()
    chars = np.zeros((x.size, 7), dtype=np.uint8)
    live = np.zeros((x.size, 7), dtype=bool)
    alive = np.ones(x.size, dtype=bool)
    for k in range(7):
        c = x & 0x1f
        x >>= 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, k] = (c | np.where(more, 0x20, 0)) + 48
        live[:, k] = alive
        alive = alive & more
    return chars, live


def _deltas(counts, index):
    """counts[i] - counts[i - 2] where the index of the count inside its mask is > 2."""
    back = np.zeros_like(counts)
    back[2:] = counts[:-2]
    return counts - np.where(index > 2, back, 0)


def counts_to_string(counts) -> str:
    """The COCO string of a list of run lengths."""
    c = np.asarray(list(counts), dtype=np.int64)
    if c.size == 0:
        return ""
    chars, live = _delta_chars(_deltas(c, np.arange(c.size)))
    return chars[live].tobytes().decode("ascii")


def string_to_counts(s) -> list:
    """The inverse of :func:`counts_to_string`."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def _split(buf, offsets, H, W):
    """bytes of all masks + (M + 1) offsets -> the list of RLE dicts."""
    raw = buf.tobytes()
    return [{"size": [H, W], "counts": raw[a:b].decode("ascii")} for a, b in zip(offsets[:-1], offsets[1:])]


# -------------------------------------------------------------------------------------------------------------------
# host definition
# -------------------------------------------------------------------------------------------------------------------
def _unpack_bits(words, width):
    """(M, H, words) int32 numpy -> (M, H, width) bool: bit x % 32 of word x // 32."""
    w = words.astype(np.int64) & 0xffffffff
    bits = (w[..., None] >> np.arange(32, dtype=np.int64)) & 1
    return bits.reshape(*words.shape[:-1], -1)[..., :width].astype(bool)


def _encode_host(masks):
    """masks (M, H, W) bool numpy -> list of RLE dicts."""
    M, H, W = masks.shape
    N = H * W
    flat = masks.transpose(0, 2, 1).reshape(M, N)
    change = flat.copy()
    change[:, 1:] = flat[:, 1:] != flat[:, :-1]                     # column 0 compares with the virtual 0
    mi, pos = np.nonzero(change)                                    # sorted by mask, then position
    k = np.bincount(mi, minlength=M)
    first = np.concatenate(([0], np.cumsum(k + 1)))                 # every mask: its transitions, then H * W
    total = int(first[-1])
    closing = np.zeros(total, dtype=bool)
    closing[first[1:] - 1] = True
    t = np.empty(total, dtype=np.int64)
    t[closing] = N
    t[~closing] = pos
    index = np.arange(total) - np.repeat(first[:-1], k + 1)
    prev = np.zeros_like(t)
    prev[1:] = t[:-1]
    counts = t - np.where(index > 0, prev, 0)
    chars, live = _delta_chars(_deltas(counts, index))
    ends = np.concatenate(([0], np.cumsum(live.sum(1))))
    return _split(chars[live], ends[first].tolist(), H, W)


# -------------------------------------------------------------------------------------------------------------------
# device path
# -------------------------------------------------------------------------------------------------------------------
def _char_bound(n, N):
    """An upper bound of the string length of a mask with n counts over N pixels, from these two numbers alone.

    A count c >= 0 takes L(c) characters, the smallest k with c < 2^(5k - 1).  The delta d = a - b of two counts
    takes at most max(L(a), L(b)): d <= a when d >= 0 and -d <= b < 2^(5 L(b) - 1) when d < 0.  So run i <= 2
    takes L(counts[i]) and run i > 2 at most L(counts[i]) + L(counts[i - 2]) - 1, in all at most
    2 S - max(n - 3, 0) with S = sum L(counts[i]).  At most N / 2^(5k - 1) of the n counts reach 2^(5k - 1), which
    bounds S by n + sum_k min(n, N // 2^(5k - 1))."""
    S = n + sum(min(n, N // lim) for lim in _GROUP_LIMITS)
    return 2 * S - max(n - 3, 0)


def _encode_device(src, form, width, plane_index=None, num_masks=None, extra=None):
    """src: a HIP tensor (P, H, row) with unit stride along the row, uint8 / bool (form bytes) or int32 words
    (form bits); mask m is plane plane_index[m] (device int32, clamped by the kernel) or plane m.  ``extra`` is a
    device int64 tensor that rides to the host with the first copy.  -> (list of RLE dicts, extra on the host)."""
    P, H = src.shape[0], src.shape[1]
    W = int(width)
    M = P if plane_index is None else int(num_masks)
    dev = src.device
    st = _native.stream(src)
    idx_ptr = _native.ptr(plane_index)
    geom = (src.data_ptr(), form, idx_ptr, P, M, H, W, src.stride(1), src.stride(0))
    counts = torch.empty(M * W, dtype=torch.int32, device=dev)
    _native.call("m2f_rle_col_counts", *geom, counts.data_ptr(), st)
    col_start = torch.zeros(M * W + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=col_start[1:])
    first = col_start[::W] + torch.arange(M + 1, dtype=torch.int64, device=dev)   # first slot of every mask
    head = first if extra is None else torch.cat([first, extra.to(torch.int64).flatten()])
    head = head.cpu()                                               # copy 1: O(M) integers, sizes the buffers
    first_h = head[:M + 1].tolist()
    extra_h = head[M + 1:]
    total = first_h[-1]                                             # runs + M
    positions = torch.empty(total, dtype=torch.int32, device=dev)
    _native.call("m2f_rle_positions", *geom, col_start.data_ptr(), positions.data_ptr(), total, st)
    delta = torch.empty(total, dtype=torch.int32, device=dev)
    nchar = torch.empty(total, dtype=torch.uint8, device=dev)
    _native.call("m2f_rle_deltas", positions.data_ptr(), col_start.data_ptr(), M, W, total, delta.data_ptr(),
                 nchar.data_ptr(), st)
    char_end = torch.cumsum(nchar, 0, dtype=torch.int64)
    # the string lengths are known on the device only; the host sizes the copy by its bound (see _char_bound)
    cap = sum(_char_bound(b - a, H * W) for a, b in zip(first_h[:-1], first_h[1:]))
    head_bytes = 8 * (M + 1)
    out = torch.empty(head_bytes + cap, dtype=torch.uint8, device=dev)
    ends = torch.cat([char_end.new_zeros(1), char_end])[first]      # (M + 1) byte offsets
    out[:head_bytes] = ends.view(torch.uint8)
    _native.call("m2f_rle_chars", delta.data_ptr(), nchar.data_ptr(), char_end.data_ptr(), total,
                 out.data_ptr() + head_bytes, cap, st)
    host = out.cpu().numpy()                                        # copy 2: offsets and encoded bytes
    offsets = host[:head_bytes].view(np.int64).tolist()
    if offsets[-1] > cap:
        raise _native.NativeError(f"rle_encode: {offsets[-1]} characters exceed the bound {cap}")
    return _split(host[head_bytes:head_bytes + offsets[-1]], offsets, H, W), extra_h


def _planes(masks, H, row):
    """(..., H, row) -> (P, H, row) with unit stride along the row, as a view where the strides allow it."""
    if masks.stride(-1) != 1 and masks.shape[-1] > 1:
        masks = masks.contiguous()
    try:
        return masks.view(-1, H, row)
    except RuntimeError:
        return masks.reshape(-1, H, row)


def rle_encode(masks, width=None) -> list:
    """masks (..., H, W) bool / uint8 (non-zero = set), or (..., H, ceil(width / 32)) int32 bit words (bit x % 32
    of word x // 32, see ``pack_mask_bits``) when ``width`` is given -> one ``{"size": [H, W], "counts": str}`` per
    mask, the leading dimensions flattened.  A HIP tensor is encoded on the device, in place (a crop view is read
    through its strides), a CPU tensor by the host definition."""
    if not torch.is_tensor(masks) or masks.dim() < 2:
        raise ValueError("masks must be a tensor of at least two dimensions")
    H, row = int(masks.shape[-2]), int(masks.shape[-1])
    if width is None:
        if masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"masks must be bool or uint8 (or int32 bit words with width=), got {masks.dtype}")
        form, W = _BYTES, row
    else:
        W = int(width)
        if masks.dtype != torch.int32 or W <= 0 or row != (W + 31) // 32:
            raise ValueError("bit masks must be int32 of ceil(width / 32) words per row")
        form = _BITS
    if H <= 0 or W <= 0:
        raise ValueError("empty masks have no encoding")
    if H * W >= 2 ** 31:
        raise ValueError(f"{H} x {W} pixels do not fit a 32-bit count")
    if masks.numel() == 0:
        return []
    if masks.device.type == "cuda":
        src = _planes(masks.detach(), H, row)
        if form == _BYTES and src.dtype == torch.bool:
            src = src.view(torch.uint8)
        return _encode_device(src, form, W)[0]
    m = masks.detach().reshape(-1, H, row).numpy()
    return _encode_host(_unpack_bits(m, W) if form == _BITS else m != 0)


# -------------------------------------------------------------------------------------------------------------------
# host readers
# -------------------------------------------------------------------------------------------------------------------
def rle_decode(rle) -> torch.Tensor:
    """RLE dict -> (H, W) bool tensor."""
    H, W = rle["size"]
    counts = np.asarray(string_to_counts(rle["counts"]), dtype=np.int64)
    if counts.sum() != H * W or (counts < 0).any():
        raise ValueError("counts do not add up to the mask size")
    flat = np.repeat(np.arange(counts.size) % 2 == 1, counts)
    return torch.from_numpy(np.ascontiguousarray(flat.reshape(W, H).T))


def rle_area(rle) -> int:
    """The number of set pixels."""
    return int(sum(string_to_counts(rle["counts"])[1::2]))
