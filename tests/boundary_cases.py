"""The cases of the boundary tests: the smallest shapes at which ``m2f_bits_boundary_ragged`` can still go wrong,
shared by test_boundary_cpu.py and test_boundary_gpu.py.  The tile constants come from the library's query, so the
heights and the width "just above a tile" follow the kernel.  The oracle planes are computed once per case
(``expected``) and never modified."""
import functools

import numpy as np

import boundary_ref
from bm2f_amd.mask_boundary import boundary_tiles
from bm2f_amd.mask_iou import _pack_rows

BAND, TILE_WORDS, D_MAX = boundary_tiles()
# the widths of the issue and one just above a column tile (a second workgroup per band, halo words on both sides)
WIDTHS = [1, 20, 31, 32, 33, 64, 65, 100, 32 * TILE_WORDS + 1]
HEIGHTS = [1, 3, 40, BAND + 1, 2 * BAND + 3]
DILATIONS = [1, 2, 3, 31, 32, 33, 64, D_MAX]


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), dtype=bool)
    m[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = True
    return m


def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def noise(H, W, seed, p=0.97):
    """Per-pixel noise, dense enough that small windows survive."""
    return np.random.RandomState(seed).rand(H, W) < p


def blobs(H, W, seed):
    rng = np.random.RandomState(seed)
    m = np.zeros((H, W), dtype=bool)
    for _ in range(4):
        m |= ellipse(H, W, rng.randint(0, H), rng.randint(0, W), rng.randint(1, H // 2 + 2), rng.randint(1, W // 2 + 2))
    return m


def _cases():
    out = []

    def add(name, mask, d):
        assert mask.dtype == bool and 1 <= d <= D_MAX
        out.append((name, mask, int(d)))

    # every height x every width, the dilations and four kinds of content dealt round robin: d >= H, d >= W and d
    # larger than both occur (H = 1, W = 1), as do d < 32 <= W and d >= 32 crossing whole words
    i = 0
    for H in HEIGHTS:
        for W in WIDTHS:
            d = DILATIONS[(i + i // len(DILATIONS)) % len(DILATIONS)]
            kind = i % 4
            mask = (noise(H, W, i), blobs(H, W, i), np.ones((H, W), dtype=bool),
                    rect(H, W, 0, H, 0, W) & ~rect(H, W, H // 2, H // 2 + 1, W // 2, W // 2 + 1))[kind]
            add(f"grid-{H}x{W}-d{d}-k{kind}", mask, d)
            i += 1
    assert any(d >= H and d >= W for _, m, d in out for H, W in [m.shape])
    assert any(d >= H and d < W for _, m, d in out for H, W in [m.shape])
    assert any(d < H and d >= W for _, m, d in out for H, W in [m.shape])

    # the contents of the issue at every dilation, on a shape with room for a 2d + 1 rectangle, more than one band,
    # a width off the word grid
    for d in DILATIONS:
        H, W = max(2 * BAND + 3, 2 * d + 9), max(100, 2 * d + 41)
        add(f"empty-d{d}", np.zeros((H, W), dtype=bool), d)
        add(f"full-d{d}", np.ones((H, W), dtype=bool), d)              # the boundary is a frame d thick
        one = np.zeros((H, W), dtype=bool)
        one[H // 2, W // 2] = True
        add(f"pixel-d{d}", one, d)
        add(f"borders-d{d}", rect(H, W, 0, H, 0, W) & ~ellipse(H, W, H / 2, W / 2, H / 5, W / 5), d)
        add(f"thick2d-rows-d{d}", rect(H, W, 3, 3 + 2 * d, 0, W), d)   # 2d rows: nothing survives
        add(f"thick2d1-rows-d{d}", rect(H, W, 3, 4 + 2 * d, 0, W), d)  # 2d + 1 rows: one row survives
        add(f"thick2d-cols-d{d}", rect(H, W, 0, H, 5, 5 + 2 * d), d)
        add(f"thick2d1-cols-d{d}", rect(H, W, 0, H, 5, 6 + 2 * d), d)
        hole = max(1, d // 2)
        add(f"hole-d{d}", ~rect(H, W, 3, 3 + hole, 3, 3 + hole), d)   # a hole smaller than d near a corner
        add(f"ellipse-d{d}", ellipse(H, W, BAND, 32, 0.45 * H, 0.45 * W), d)   # across a band edge and a word edge
        add(f"blobs-d{d}", blobs(H, W, 100 + d), d)
        add(f"noise-d{d}", noise(H, W, 200 + d, p=1 - 0.5 / (2 * d + 1) ** 2), d)
    assert all(W > 2 * d and H > 2 * d for n, m, d in out if not n.startswith("grid") for H, W in [m.shape])
    return out


CASES = _cases()
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def expected(index, d=None):
    """The oracle's boundary of case ``index`` at its own dilation (or ``d``) as packed rows; computed once."""
    _, mask, own = CASES[index]
    plane = _pack_rows(boundary_ref.boundary(mask, own if d is None else d))
    plane.setflags(write=False)
    return plane


def pack_plane(mask, hostile=True):
    """(H, W) bool -> (H, words) int32; with ``hostile`` the bits x >= W of every row's last word are ones."""
    W = mask.shape[1]
    p = _pack_rows(mask).copy()
    if hostile and W % 32:
        p[:, -1] |= np.int32(-(1 << (W % 32)))
    return p


def pack_batch(masks, hostile=True, align=4):
    """Dense masks -> (words (N,) int32 numpy, offsets (M,), sizes (M, 2)) in the ragged layout.  With ``hostile``
    the bits x >= W of every row's last word are ones and so are the padding words in front of, between and behind the planes:
    a kernel that uses any of them gives a wrong plane."""
    fill = -1 if hostile else 0
    parts, offsets, sizes, at = [np.full(align, fill, dtype=np.int32)], [], [], align
    for m in masks:
        H, W = m.shape
        p = pack_plane(m, hostile)
        pad = (-at) % align
        parts.append(np.full(pad, fill, dtype=np.int32))
        at += pad
        offsets.append(at)
        sizes.append((H, W))
        parts.append(p.reshape(-1))
        at += p.size
    parts.append(np.full(3, fill, dtype=np.int32))
    return np.concatenate(parts), np.asarray(offsets, dtype=np.int64), np.asarray(sizes, dtype=np.int64)


def planes_of(words, offsets, sizes):
    """The (H, words) planes of a flat buffer, as numpy views."""
    words = np.asarray(words)
    out = []
    for o, (H, W) in zip(offsets, sizes):
        wr = (W + 31) // 32
        out.append(words[o:o + H * wr].reshape(H, wr))
    return out


# -------------------------------------------------------------------------------------------------------------------
# the checks both test files run, on the CPU restatement and on the kernel
# -------------------------------------------------------------------------------------------------------------------
def check_planes(got_words, offsets, sizes, indices, dilations=None):
    """Every plane equals the oracle's packed rows bit for bit; the output tail bits are zero."""
    for k, (i, plane) in enumerate(zip(indices, planes_of(got_words, offsets, sizes))):
        want = expected(i, None if dilations is None else int(dilations[k]))
        assert plane.shape == want.shape and np.array_equal(plane, want), CASES[i][0]
        W = CASES[i][1].shape[1]
        if W % 32:
            assert not (plane[:, -1].view(np.uint32) >> np.uint32(W % 32)).any(), CASES[i][0]


def run_ragged(indices, device, hostile=True, dilations="own", align=4):
    """boundary_bits_ragged of the cases ``indices`` in one batch -> (host words, offsets, sizes)."""
    import torch
    from bm2f_amd import boundary_bits_ragged
    words, offsets, sizes = pack_batch([CASES[i][1] for i in indices], hostile=hostile, align=align)
    d = [CASES[i][2] for i in indices] if isinstance(dilations, str) else dilations
    t = torch.from_numpy(words).to(device)
    keep = t.clone()
    out = boundary_bits_ragged(t, offsets, sizes, dilations=d)
    assert out.device == t.device and out.dtype == torch.int32 and out.shape == t.shape
    assert torch.equal(t, keep)                                       # the input is left as it was
    return out.cpu().numpy(), offsets, sizes
