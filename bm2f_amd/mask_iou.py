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
:func:`rle_to_bits_ragged`, :func:`mask_pair_counts_ragged`
                          the same for masks of many images of different sizes in one flat word buffer: one launch
                          of ``m2f_rle_decode_bits_ragged`` / ``m2f_bits_pair_counts_ragged`` whatever the number of
                          images, dealt to workgroups by host-built tables (the COCO evaluator's batch step).

On CPU tensors a numpy restatement of the same definitions runs; that is not a fallback: on a HIP tensor a kernel
error raises ``NativeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native

_MAX_MASKS = 65535                     # m2f_rle_decode_bits: masks per launch
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def pair_tiles():
    """(TA, TB, chunk_words) of ``m2f_bits_pair_counts``: the instance tile and the word positions of a workgroup."""
    return _native.query("m2f_bits_pair_tiles", outs="iii")


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


def _check_size(H, W, where=""):
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"{where}{H} x {W} pixels: sizes must be positive and fit a 32-bit count")


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
    _check_size(H, W)
    positions, offsets = _run_ends_sized(rles, np.full(len(rles), H * W, dtype=np.int64))
    return positions, offsets, H, W


def _run_ends_sized(rles, pixels):
    """-> (positions, offsets) of masks whose counts must add up to ``pixels[m]``."""
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
    if (n[present] == 0).any() or (ends[offsets[1:][present] - 1] != pixels[present]).any():
        raise ValueError("counts do not add up to the mask size")
    return ends.astype(np.int32), offsets


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
    dev = _native.upload_tables({"offsets": offsets, "positions": positions}, device)  # one copy
    off, pos = dev["offsets"], dev["positions"]
    out = torch.empty((M, H, (W + 31) // 32), dtype=torch.int32, device=device)
    st = _native.stream(device)
    with torch.cuda.device(device):
        for m0 in range(0, M, _MAX_MASKS):
            m1 = min(M, m0 + _MAX_MASKS)
            _native.call("m2f_rle_decode_bits", _native.ptr_or_null(pos), pos.numel(),
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
    # the query reports a multiple of 4 bytes
    work = _native.workspace("m2f_bits_pair_workspace", Da, Db, T, H, W, device=dev, dtype=torch.int32, unit=4)
    out = torch.empty(Da * Db + (Da + Db) * T, dtype=torch.int64, device=dev)
    n0, n1 = Da * Db, Da * Db + Da * T
    with torch.cuda.device(dev):
        _native.call("m2f_bits_pair_counts", a.data_ptr(), Da, sa, b.data_ptr(), Db, sb, T, H, W, out.data_ptr(),
                     out[n0:].data_ptr(), out[n1:].data_ptr(), work.data_ptr(), work.numel() * 4, _native.stream(dev))
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


# -------------------------------------------------------------------------------------------------------------------
# ragged forms: masks of many images of different sizes in one flat word buffer
# -------------------------------------------------------------------------------------------------------------------
_PLANE_ALIGN = 4                        # words: planes start on 16 bytes so that the pair kernel loads 128 bits
_GROUP_FIELDS = 8                       # M2F_RAGGED_GROUP_FIELDS
MAX_RAGGED_WORDS = 2 ** 31 - 1          # m2f_bits_pair_counts_ragged keeps plane offsets in 32 bits


def _ragged_sizes(rles, sizes):
    """-> (M, 2) int64 (H, W) per mask from the masks' own ``size`` and, for ``None`` entries, from ``sizes``."""
    if sizes is not None and len(sizes) != len(rles):
        raise ValueError(f"{len(sizes)} sizes for {len(rles)} masks")
    out = np.zeros((len(rles), 2), dtype=np.int64)
    for m, r in enumerate(rles):
        given = None if sizes is None or sizes[m] is None else [int(v) for v in sizes[m]]
        own = None if r is None else [int(v) for v in r["size"]]
        if own is None and given is None:
            raise ValueError(f"mask {m} is None and sizes does not give its (H, W)")
        if own is not None and given is not None and own != given:
            raise ValueError(f"mask {m} has size {own}, {given} was expected")
        H, W = own if own is not None else given
        _check_size(H, W)
        out[m] = (H, W)
    return out


def _plane_words(sizes):
    return sizes[:, 0] * ((sizes[:, 1] + 31) // 32)


_PARSE_CHUNK = 1 << 20                  # characters (or list entries) parsed at a time


def _run_ends_chunked(rles, pixels):
    """``_run_ends_sized`` over runs of masks of about ``_PARSE_CHUNK`` characters: the vectorised parser keeps a
    dozen int64 temporaries per character, and parsing a whole batch of dense masks at once was measured 1.3x slower
    than parsing it image by image."""
    size = np.array([0 if r is None else len(r["counts"]) for r in rles], dtype=np.int64)
    cuts = [0]
    used = 0
    for m, n in enumerate(size):
        if used and used + n > _PARSE_CHUNK:
            cuts.append(m)
            used = 0
        used += n
    cuts.append(len(rles))
    if len(cuts) == 2:
        return _run_ends_sized(rles, pixels)
    parts = [_run_ends_sized(rles[a:b], pixels[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    base = np.concatenate(([0], np.cumsum([p.size for p, _ in parts])))[:-1]
    offsets = np.concatenate([o[:-1] + s for (_, o), s in zip(parts, base)] + [[base[-1] + parts[-1][1][-1]]])
    return np.concatenate([p for p, _ in parts]), offsets.astype(np.int64)


def _decode_plan(rles, sizes):
    """Every check of rle_to_bits_ragged -> (hw (M, 2) int64, out_offsets (M,) int64, total words, the tables of
    ``m2f_rle_decode_bits_ragged`` as int64-aligned host arrays)."""
    hw = _ragged_sizes(rles, sizes)
    positions, offsets = _run_ends_chunked(rles, hw[:, 0] * hw[:, 1])
    padded = (_plane_words(hw) + _PLANE_ALIGN - 1) // _PLANE_ALIGN * _PLANE_ALIGN
    out_offsets = np.concatenate(([0], np.cumsum(padded)))[:-1].astype(np.int64)
    total = int(padded.sum())
    if total > MAX_RAGGED_WORDS:
        raise ValueError(f"the planes take {total} words, more than the {MAX_RAGGED_WORDS} of one buffer; "
                         "split the masks over several calls")
    nblk =(hw[:, 1] + 255) // 256
    mask_of = np.repeat(np.arange(len(rles), dtype=np.int64), nblk)
    first = np.concatenate(([0], np.cumsum(nblk)))[:-1]
    blocks = np.stack((mask_of, np.arange(mask_of.size) - first[mask_of]), axis=1).astype(np.int32)
    tables = {"offsets": offsets, "out_offsets": out_offsets, "sizes": hw.astype(np.int32), "blocks": blocks,
              "positions": positions}
    return hw, out_offsets, total, tables


def _launch_decode(dev_tables, num_masks, words, device):
    t = dev_tables
    with torch.cuda.device(device):
        _native.call("m2f_rle_decode_bits_ragged", _native.ptr_or_null(t["positions"]), t["positions"].numel(),
                     t["offsets"].data_ptr(), num_masks, t["sizes"].data_ptr(), t["out_offsets"].data_ptr(),
                     _native.ptr_or_null(t["blocks"]), t["blocks"].numel() // 2, _native.ptr_or_null(words),
                     words.numel(), _native.stream(device))


def rle_to_bits_ragged(rles, device=None, sizes=None):
    """RLE dicts of any sizes (``counts`` as in :func:`rle_to_bits`; an entry may be ``None``, a zero plane whose
    (H, W) ``sizes[m]`` gives) -> ``(words, offsets, sizes)``: ``words`` a flat int32 tensor on ``device``, mask
    ``m`` occupying ``H_m * ceil(W_m / 32)`` words at ``offsets[m]`` in the layout of ``pack_mask_bits`` with zero
    tail bits; ``offsets`` (M,) int64 and ``sizes`` (M, 2) int64 host arrays.  Planes start on multiples of 4 words
    (16 bytes), which lets ``mask_pair_counts_ragged`` load 128 bits at a time; the padding words between planes are
    unspecified on the device (zero on the CPU) and every consumer here ignores them.  On a HIP device one upload
    and one launch of ``m2f_rle_decode_bits_ragged`` whatever the number of masks and sizes.

    Raises ValueError, before any launch, on what :func:`rle_to_bits` refuses, when a mask's size contradicts
    ``sizes`` or a ``None`` entry has none, and when the planes take more than ``MAX_RAGGED_WORDS`` words."""
    device = torch.device("cpu" if device is None else device)
    rles = list(rles)
    if not rles:
        return torch.zeros(0, dtype=torch.int32, device=device), np.zeros(0, np.int64), np.zeros((0, 2), np.int64)
    hw, out_offsets, total, tables = _decode_plan(rles, sizes)
    if device.type != "cuda":
        words = np.zeros(total, dtype=np.int32)
        pos, off = tables["positions"], tables["offsets"]
        for m, (H, W) in enumerate(hw):
            plane = _decode_host(pos[off[m]:off[m + 1]], np.array([0, off[m + 1] - off[m]]), int(H), int(W))
            words[out_offsets[m]:out_offsets[m] + plane.size] = plane.reshape(-1)
        return torch.from_numpy(words).to(device), out_offsets, hw
    dev = _native.upload_tables(tables, device)
    words = torch.empty(total, dtype=torch.int32, device=device)
    _launch_decode(dev, len(rles), words, device)
    return words, out_offsets, hw


def _pair_plan(groups, total_words):
    """Every check of mask_pair_counts_ragged -> (per-group (na, nb), the tables of ``m2f_bits_pair_counts_ragged``,
    number of tile rows)."""
    TA, TB, CHUNK = pair_tiles()
    G = len(groups)
    desc = np.zeros((G, _GROUP_FIELDS), dtype=np.int64)
    a_all, b_all, tiles = [], [], []
    a0 = b0 = i0 = t0 = 0
    for g, grp in enumerate(groups):
        try:
            H, W, a_off, b_off = grp
            H, W = int(H), int(W)
            a_off = np.asarray(a_off, dtype=np.int64).reshape(-1)
            b_off = np.asarray(b_off, dtype=np.int64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"group {g} must be (H, W, a_offsets, b_offsets)") from e
        _check_size(H, W, f"group {g}: ")
        fw = H * ((W + 31) // 32)
        for off in (a_off, b_off):
            if off.size and (off.min() < 0 or off.max() + fw > total_words):
                raise ValueError(f"group {g}: a plane of {fw} words does not fit the buffer of {total_words}")
        na, nb = a_off.size, b_off.size
        desc[g] = (H, W, na, nb, a0, b0, i0, t0)
        a_all.append(a_off)
        b_all.append(b_off)
        if na or nb:
            ta, tb, ch = max(1, -(-na // TA)), max(1, -(-nb // TB)), -(-fw // CHUNK)
            idx = np.arange(ta * tb * ch, dtype=np.int64)
            tiles.append(np.stack((np.full(idx.size, g), idx // (tb * ch), idx // ch % tb, idx % ch), axis=1))
            t0 += idx.size
        a0, b0, i0 = a0 + na, b0 + nb, i0 + na * nb
    tables = {"groups": desc,
              "a_off": np.concatenate(a_all) if a_all else np.zeros(0, np.int64),
              "b_off": np.concatenate(b_all) if b_all else np.zeros(0, np.int64),
              "tiles": (np.concatenate(tiles) if tiles else np.zeros((0, 4), np.int64)).astype(np.int32)}
    return desc, tables, t0


def _pair_counts_ragged_host(words, desc, tables):
    out = []
    for H, W, na, nb, a0, b0, _, _ in desc:
        wr = (W + 31) // 32
        fw = H * wr

        def planes(offs):
            if offs.size == 0:
                return np.zeros((0, 1, H, wr), dtype=np.int32)
            return np.stack([words[o:o + fw] for o in offs]).reshape(-1, 1, H, wr)
        a = planes(tables["a_off"][a0:a0 + na])
        b = planes(tables["b_off"][b0:b0 + nb])
        inter, area_a, area_b = _pair_counts_host(a, b, int(W))
        out.append((inter.reshape(na, nb), area_a.reshape(na), area_b.reshape(nb)))
    return out


def _split_counts(host, desc):
    """The flat output [inter | area_a | area_b] -> one (inter (na, nb), area_a (na,), area_b (nb,)) per group."""
    n_inter = int((desc[:, 2] * desc[:, 3]).sum())
    n_a = int(desc[:, 2].sum())
    out = []
    for _, _, na, nb, a0, b0, i0, _ in desc:
        out.append((host[i0:i0 + na * nb].reshape(na, nb), host[n_inter + a0:n_inter + a0 + na],
                    host[n_inter + n_a + b0:n_inter + n_a + b0 + nb]))
    return out


def _launch_pairs(words, desc, dev_tables, num_tiles, device):
    """-> the device int64 output [inter | area_a | area_b]."""
    n_inter = int((desc[:, 2] * desc[:, 3]).sum())
    n_a, n_b = int(desc[:, 2].sum()), int(desc[:, 3].sum())
    work = _native.workspace("m2f_bits_pair_ragged_workspace", num_tiles, device=device, dtype=torch.int32, floor=4,
                             unit=4)
    out = torch.empty(max(n_inter + n_a + n_b, 1), dtype=torch.int64, device=device)
    t = dev_tables
    with torch.cuda.device(device):
        _native.call("m2f_bits_pair_counts_ragged", _native.ptr_or_null(words), words.numel(), t["groups"].data_ptr(),
                     desc.shape[0], _native.ptr_or_null(t["a_off"]), n_a, _native.ptr_or_null(t["b_off"]), n_b,
                     _native.ptr_or_null(t["tiles"]), num_tiles, n_inter, out.data_ptr(), out.data_ptr() + 8 * n_inter,
                     out.data_ptr() + 8 * (n_inter + n_a), work.data_ptr(), work.numel() * 4, _native.stream(device))
    return out[:n_inter + n_a + n_b]


def mask_pair_counts_ragged(words, groups):
    """words: a flat int32 tensor of bit planes (as :func:`rle_to_bits_ragged` returns; any word offsets are
    accepted, 16-byte aligned ones are read 128 bits at a time); groups: one ``(H, W, a_offsets, b_offsets)`` per
    image, the word offsets of its ``na`` detection planes and ``nb`` ground-truth planes of ``H x W`` pixels (either
    may be empty).  -> one ``(inter (na, nb), area_a (na,), area_b (nb,))`` of host int64 arrays per group; set tail
    bits are ignored.  On a HIP tensor one upload of the tables, the two launches of ``m2f_bits_pair_counts_ragged``
    whatever the number of groups, and one device-to-host copy.

    Raises ValueError, before any launch, when a group is malformed, a size is not positive, a plane does not lie
    inside ``words`` or ``words`` holds more than ``MAX_RAGGED_WORDS`` words."""
    if not torch.is_tensor(words) or words.dim() != 1 or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("words must be a flat contiguous int32 tensor")
    if words.numel() > MAX_RAGGED_WORDS:
        raise ValueError(f"words holds {words.numel()} words, more than the {MAX_RAGGED_WORDS} of one call")
    groups = list(groups)
    if not groups:
        return []
    desc, tables, num_tiles = _pair_plan(groups, words.numel())
    if words.device.type != "cuda":
        return _pair_counts_ragged_host(words.detach().numpy(), desc, tables)
    dev = _native.upload_tables(tables, words.device)
    out = _launch_pairs(words.detach(), desc, dev, num_tiles, words.device)
    return _split_counts(out.cpu().numpy(), desc)                     # the one copy


def _groups_by_offset(groups, hw, out_offsets):
    """Groups ``(H, W, a_masks, b_masks)`` of indices into a batch of masks of sizes ``hw`` at ``out_offsets`` ->
    the ``(H, W, a_offsets, b_offsets)`` of mask_pair_counts_ragged, with the checks of the indices."""
    by_offset = []
    for g, (H, W, ia, ib) in enumerate(groups):
        ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1), np.asarray(ib, dtype=np.int64).reshape(-1)
        for idx in (ia, ib):
            if idx.size and (idx.min() < 0 or idx.max() >= hw.shape[0]):
                raise ValueError(f"group {g} names masks outside the batch")
            if idx.size and ((hw[idx, 0] != int(H)) | (hw[idx, 1] != int(W))).any():
                raise ValueError(f"group {g}: a mask's size is not the group's {int(H)} x {int(W)}")
        by_offset.append((H, W, out_offsets[ia], out_offsets[ib]))
    return by_offset


def rle_pair_counts_ragged(rles, groups, device=None, sizes=None):
    """:func:`rle_to_bits_ragged` and :func:`mask_pair_counts_ragged` of one batch with a single upload: ``groups``
    holds ``(H, W, a_masks, b_masks)`` with *indices into* ``rles`` in place of word offsets.  -> the per-group
    counts.  On a HIP device: one upload, one decode launch, one pair-count call and one copy (the evaluator's
    batch step)."""
    device = torch.device("cpu" if device is None else device)
    rles = list(rles)
    groups = list(groups)
    if not groups:
        return []
    if not rles:
        return [(np.zeros((0, 0), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in groups]
    hw, out_offsets, total, dtables = _decode_plan(rles, sizes)
    desc, ptables, num_tiles = _pair_plan(_groups_by_offset(groups, hw, out_offsets), total)
    if device.type != "cuda":
        words = rle_to_bits_ragged(rles, device, sizes)[0]
        return _pair_counts_ragged_host(words.numpy(), desc, ptables)
    dev = _native.upload_tables({**dtables, **ptables}, device)
    words = torch.empty(total, dtype=torch.int32, device=device)
    _launch_decode(dev, len(rles), words, device)
    out = _launch_pairs(words, desc, dev, num_tiles, device)
    return _split_counts(out.cpu().numpy(), desc)                     # the one copy
