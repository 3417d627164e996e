"""Masked-attention inputs with a trained decoder's score ranges (tens to over a hundred log2 units per row), for
tests/test_attn_range_cpu.py and tests/test_attn_range_gpu.py.  Plain helpers: no fixtures, no GPU.

The kernel (bm2f_amd/csrc/decoder.hip) works in the log2 domain on s * scale * log2(e).  With ``torch.randn`` queries
and keys those scores have unit variance and the row maxima of two 64-key blocks differ by 1 to 3, so the lazy
rescale (kLazyLog2 = 8), the chunk combine's underflowing weights and the backward's 2^(s - lse) at large |s| never
act.  :func:`make_case` builds, per head h with a random unit vector u[h],

    k[j, h, :] = a[j] * ka * u[h] + 0.3 * randn_perp   ka = 1 / 32          (randn_perp: randn minus its part along u[h])
    q[i, h, :] = c[i] * qa * u[h] + 0.3 * randn        qa = 1 / (ka * scale * log2 e)  ~ 125

so the log2-domain score of (i, j) is about c[i] * a[j]: a[j] = profile(j // 64) + 2 randn steps from one 64-key block
to the next, and c[i] = +1 / -1 on even / odd rows (0.5 on rows 2, 7, 12, ...) gives the neighbouring rows of one
16-row MFMA tile opposite profiles, so one row of a wave needs the rescale where the next does not.  The magnitude
sits in q and k stays small: dq = dS @ k then has no large cancelling terms (with large keys an ideal 16-bit backward
misses the project's gradient tolerance by itself).
"""
import math

import torch

LOG2E = 1.4427
HEAD_DIM = 32
SCALE = HEAD_DIM ** -0.5
KA = 1.0 / 32
QA = 1.0 / (KA * SCALE * LOG2E)
BLOCK = 64                      # keys per block of the forward kernel
LAZY_LOG2 = 8.0                 # decoder.hip kLazyLog2
SPIKE_KEYS = 4

PROFILES = ("up", "down", "slow", "spike")
# Seeds of the (48, 640) cases.  The 2-unit jitter of a[j] moves a block's max by about one unit, so of the 12-unit
# steps of ``up`` / ``down`` one in a thousand lands below the threshold of 8: these are seeds (about half of all) at
# which every step of the c = +-1 rows clears it, as tests/test_attn_range_cpu.py asserts.
SEEDS = {"up": 1, "down": 1, "slow": 1, "spike": 1}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# rows of make_case's mask with a special pattern (both signs of c: rows 3 and 5 have c = -1, row 4 has c = +1)
ROW_LAST_ONLY, ROW_FIRST_ONLY, ROW_OPEN = 3, 4, 5


def row_coeff(Lq):
    """c[i]: +1 on even rows, -1 on odd rows, 0.5 on rows 2, 7, 12, ..."""
    c = torch.ones(Lq, dtype=torch.float64)
    c[1::2] = -1.0
    c[2::5] = 0.5
    return c


def key_profile(profile, Lk):
    """The noise-free a[j] of a profile."""
    blk = (torch.arange(Lk) // BLOCK).double()
    if profile == "up":
        return 12.0 * blk
    if profile == "down":
        return -12.0 * blk
    if profile == "slow":
        return 6.0 * blk
    if profile == "spike":
        a = torch.zeros(Lk, dtype=torch.float64)
        s0 = spike_start(Lk)
        a[s0:s0 + SPIKE_KEYS] = 60.0
        return a
    raise ValueError(f"unknown profile {profile!r}")


def spike_start(Lk):
    return Lk // 2 + 5


def make_case(profile, dtype, Lq, Lk, H=8, seed=0):
    """-> q (1, Lq, 32 H), k, v (1, Lk, 32 H), blocked (1, Lq, Lk) bool, gout (1, Lq, 32 H), all on the CPU; the
    floating tensors hold values of ``dtype`` (rounded once; kernel and reference both start from them)."""
    g = torch.Generator().manual_seed(seed)
    C = HEAD_DIM * H

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    u = randn(H, HEAD_DIM)
    u = u / u.norm(dim=1, keepdim=True)
    c = row_coeff(Lq)
    a = key_profile(profile, Lk) + 2.0 * randn(Lk)
    # the keys' noise without its component along u[h]: against q's c * qa * u that component alone would add
    # 0.3 * qa * scale * log2(e) ~ 9.6 log2 units of per-key noise to every score and bury the 2-unit jitter of a[j]
    nk = 0.3 * randn(Lk, H, HEAD_DIM)
    nk = nk - (nk * u[None]).sum(-1, keepdim=True) * u[None]
    k = a[:, None, None] * KA * u[None] + nk
    q = c[:, None, None] * QA * u[None] + 0.3 * randn(Lq, H, HEAD_DIM)
    v = randn(Lk, C)
    gout = randn(Lq, C)
    blocked = torch.rand(Lq, Lk, generator=g) < 0.6
    blocked[:, 0] = False
    if Lq > ROW_LAST_ONLY:
        blocked[ROW_LAST_ONLY] = True
        blocked[ROW_LAST_ONLY, -1] = False
    if Lq > ROW_FIRST_ONLY:
        blocked[ROW_FIRST_ONLY] = True
        blocked[ROW_FIRST_ONLY, 0] = False
    if Lq > ROW_OPEN:
        blocked[ROW_OPEN] = False
    q, k, v, gout = (t.reshape(1, -1, C).to(dtype) for t in (q, k, v, gout))
    return q, k, v, blocked[None], gout


def log2_scores(q, k, blocked, H=8):
    """fp64 s * scale * log2(e) per head, (H, Lq, Lk), blocked entries -inf."""
    Lq, Lk = q.shape[1], k.shape[1]
    qh = q[0].double().view(Lq, H, HEAD_DIM).transpose(0, 1)
    kh = k[0].double().view(Lk, H, HEAD_DIM).transpose(0, 1)
    s = qh @ kh.transpose(1, 2) * (SCALE * math.log2(math.e))
    return s.masked_fill(blocked[0][None], float("-inf"))


def block_maxima(s, size=BLOCK):
    """(H, Lq, Lk) scores -> (H, Lq, ceil(Lk / size)) maxima over each run of ``size`` keys (-inf: none open)."""
    H, Lq, Lk = s.shape
    nb = (Lk + size - 1) // size
    pad = s.new_full((H, Lq, nb * size), float("-inf"))
    pad[..., :Lk] = s
    return pad.view(H, Lq, nb, size).amax(-1)


def max_rel(a, b):
    """The project's metric: max|a - b| / max|b|."""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()
