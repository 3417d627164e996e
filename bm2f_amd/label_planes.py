"""Integer label maps in front of the label kernels (``csrc/label_counts.hip``, ``csrc/label_rle.hip``,
``m2f_label_views``, the ``_labels`` entry points of ``csrc/point_sample.hip``): which dtypes they read and how any
other integer input becomes one of them.  No device code.

:data:`LABEL_DTYPES`       the dtypes every label kernel reads, with item bytes and range; :data:`WIDE_DTYPE` the one
                           more that the predicted side of the counting kernel reads.
:func:`as_label_plane`     one integer array or tensor -> a dtype the kernels read, in the same container.
:func:`same_dtype`         a batch -> its widest dtype (a batch is counted in one dtype per side).
:func:`as_label_maps`      the training targets' form: tensors of one dtype, contiguous.
"""
from __future__ import annotations

import numpy as np
import torch

# torch dtype -> (item bytes, least, greatest)
LABEL_DTYPES = {torch.uint8: (1, 0, 255), torch.int16: (2, -2 ** 15, 2 ** 15 - 1),
                torch.int32: (4, -2 ** 31, 2 ** 31 - 1)}
WIDE_DTYPE = torch.int64
_INT_DTYPES = (*LABEL_DTYPES, torch.int8, WIDE_DTYPE)          # what as_label_maps converts


def np_dtype(dtype):
    """A torch or numpy dtype -> the numpy dtype; ``object`` for one numpy has no name for (no label dtype)."""
    try:
        return np.dtype(str(dtype).replace("torch.", "")) if isinstance(dtype, torch.dtype) else np.dtype(dtype)
    except TypeError:
        return np.dtype(object)


_NP_DTYPES = tuple(np_dtype(d) for d in LABEL_DTYPES)


def reads(dtype, wide=False):
    """Whether the label kernels read ``dtype`` (torch or numpy) as it is; with ``wide`` int64 counts too."""
    d = np_dtype(dtype)
    return d in _NP_DTYPES or (wide and d == np_dtype(WIDE_DTYPE))


def integer_plane(x, what):
    """``x`` as it is if a tensor, else as an array; ValueError unless it holds integers (bool is none)."""
    if torch.is_tensor(x):
        integral = not (x.is_floating_point() or x.dtype == torch.bool)
    else:
        x = np.asarray(x)
        integral = x.dtype.kind in "iu"
    if not integral:
        raise ValueError(f"{what} must hold integer labels, got {x.dtype}")
    return x


def as_label_plane(x, what, *, wide=False):
    """An integer label map -> an array or tensor of a dtype the kernels read: the same object when it already is one
    (int64 too with ``wide``), else int32 in the same container.  ValueError for float or bool input and for an array
    whose labels do not fit an int32 (a tensor is converted unread: it may lie on a device)."""
    x = integer_plane(x, what)
    if reads(x.dtype, wide):
        return x
    if torch.is_tensor(x):
        return x.to(torch.int32)
    if x.size and (x.min() < -2 ** 31 or x.max() >= 2 ** 31):
        raise ValueError(f"{what} holds labels beyond int32")
    return x.astype(np.int32)


def same_dtype(planes):
    """Planes of mixed label dtypes -> all as the widest (a batch is counted in one dtype per side); the list itself
    when they already agree."""
    dtypes = [np_dtype(p.dtype) for p in planes]
    widest = max(dtypes, key=lambda d: d.itemsize, default=None)
    if all(d == widest for d in dtypes):
        return planes
    return [p if d == widest else (p.to(getattr(torch, widest.name)) if torch.is_tensor(p) else p.astype(widest))
            for p, d in zip(planes, dtypes)]


def as_label_maps(maps, what="label_map"):
    """The maps in a form the kernels read in place: (H, W) integer tensors of one dtype among uint8, int16 and int32,
    contiguous.  Maps that already share such a dtype are kept as they are; otherwise every map is converted to
    int32, once (int64, what the reference's mappers ship, lands here)."""
    maps = [m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m)) for m in maps]
    for b, m in enumerate(maps):
        if m.dim() != 2 or m.dtype not in _INT_DTYPES:
            raise ValueError(f"{what} of image {b} must be an (H, W) integer tensor, got {tuple(m.shape)} {m.dtype}")
    dtypes = {m.dtype for m in maps}
    if len(dtypes) == 1 and maps[0].dtype in LABEL_DTYPES:
        return [m.contiguous() for m in maps]
    return [m.to(torch.int32).contiguous() for m in maps]
