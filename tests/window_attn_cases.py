"""Case table and input builder of the shifted-window attention sweep (tests/test_window_attn_sweep_cpu.py and
tests/test_window_attn_sweep_gpu.py).  Plain helpers: no fixtures, no GPU.

csrc/window_attn.hip is compiled per element type and per NT = ceil(ws^2 / 16), the number of 16-token tiles (= waves)
of a window.  For the window sizes it accepts:

    ws   2  3  4   5   6   7   8   9   10   11   12
    N    4  9  16  25  36  49  64  81  100  121  144
    NT   1  1  1   2   3   4   4   6   7    8    9
    NP   32 32 32  32  64  64  64  96  128  128  160      (pad32(N), the LDS images' token count)

ws 4, 8 and 12 fill their tiles exactly (no tail keys or tail query rows); every other size has a tail.

Inputs are drawn in fp64 from a seeded CPU generator and cast: qkv ~ randn, gout ~ randn, and a bias table ~ randn,
whose O(1) entries (a fresh model's are 0.02) make a wrong bias index move the output as much as a wrong key does.
tests/test_window_attn_sweep_cpu.py asserts that: with these inputs a rolled or reversed table, a shift off by one and a
wrong scale each move the fp64 output by far more than any tolerance the GPU test can reach.
"""
from collections import namedtuple

import torch

from swin_ref import _window_pixels, window_attention_ref

HEAD_DIM = 32
SEED = 0
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# windows = (windows_y, windows_x); scale None = head_dim ** -0.5; qk_gain multiplies q and k
Case = namedtuple("Case", "group ws shift B nH windows scale qk_gain", defaults=(None, 1.0))


def tiles_of(ws):
    return (ws * ws + 15) // 16


def case_id(c):
    s = f"{c.group}-ws{c.ws}-nt{tiles_of(c.ws)}-shift{c.shift}-b{c.B}h{c.nH}-{c.windows[0]}x{c.windows[1]}"
    if c.scale is not None:
        s += f"-scale{c.scale}"
    return s


def _build_cases():
    cases = []
    for ws in range(2, 13):                       # all eight NT, both kinds of tile fill, 12 windows, nine regions
        for shift in (0, ws // 2):
            cases.append(Case("sweep", ws, shift, 2, 2, (2, 3)))
    for ws in (6, 8, 9, 11):                      # shifts other than ws // 2
        for shift in (1, ws - 1):
            cases.append(Case("shiftedge", ws, shift, 2, 2, (2, 3)))
    cases.append(Case("shiftedge", 3, 2, 2, 2, (2, 3)))     # ws 3 shift 1 is the sweep's ws // 2
    for ws in (4, 6, 10):                         # 1, 3 and 9 windows for the eight segments of wattn_dtable_kernel
        cases.append(Case("few", ws, ws // 2, 1, 1, (1, 1)))    # one window = whole map: the first slice is empty
        cases.append(Case("few", ws, ws // 2, 1, 3, (1, 3)))
        cases.append(Case("few", ws, ws // 2, 3, 3, (1, 3)))
    for ws in (6, 10):
        cases.append(Case("scale", ws, ws // 2, 2, 2, (2, 3), 0.2))
        cases.append(Case("scale", ws, ws // 2, 2, 2, (2, 3), 0.0))   # scores = bias + mask, no matmul in the way
    for ws in (3, 8, 11):                         # score sd near 16, rows nearly one-hot: a trained backbone's range
        cases.append(Case("wide", ws, ws // 2, 2, 2, (2, 3), None, 4.0))
    return cases


CASES = _build_cases()
SWEEP_SHIFTED = [c for c in CASES if c.group == "sweep" and c.shift > 0]
WIDE_DTYPES = ("fp32", "fp16")


def dtypes_of(c):
    return WIDE_DTYPES if c.group == "wide" else tuple(DTYPES)


def scale_of(c):
    return HEAD_DIM ** -0.5 if c.scale is None else c.scale


def make_inputs(c, dtype=torch.float64, seed=SEED):
    """-> qkv (B, ws wy, ws wx, 3 nH 32), gout (B, ws wy, ws wx, nH 32) in ``dtype`` and table ((2ws-1)^2, nH) in fp32
    (fp64 for dtype fp64), all on the CPU.  The same fp64 draws whatever the dtype."""
    g = torch.Generator().manual_seed(seed)
    Hp, Wp, C = c.ws * c.windows[0], c.ws * c.windows[1], c.nH * HEAD_DIM
    qkv = torch.randn(c.B, Hp, Wp, 3 * C, generator=g, dtype=torch.float64)
    table = torch.randn((2 * c.ws - 1) ** 2, c.nH, generator=g, dtype=torch.float64)
    gout = torch.randn(c.B, Hp, Wp, C, generator=g, dtype=torch.float64)
    qkv[..., :2 * C] *= c.qk_gain
    return qkv.to(dtype), table.to(torch.float64 if dtype == torch.float64 else torch.float32), gout.to(dtype)


def last_token_pixels(c):
    """(nW,) flat pixel index of token N - 1 of every window."""
    return _window_pixels(c.ws * c.windows[0], c.ws * c.windows[1], c.ws, c.shift)[:, -1]


def fill_last_tokens(c, qkv, value=1e4):
    """A copy of qkv with q, k and v of the last token of every window set to ``value``.  The kernels' tail slots
    N .. NP-1 repeat that token's table entry, so a tail key that leaked into a softmax or into dK / dV would show at
    this magnitude."""
    B, Hp, Wp, C3 = qkv.shape
    out = qkv.clone().reshape(B, Hp * Wp, C3)
    out[:, last_token_pixels(c)] = value
    return out.reshape(B, Hp, Wp, C3)


# Tail isolation runs on a single window.  A key of 1e4 scores scale * 1e4 * sum(q) against a random query, thousands
# either way, so a row is one-hot on or off that key -- unless sum(q) lands within about 1e-3 of the tie.  Such a row's
# probabilities turn on the last bits of a score of magnitude 1e4 and its gradients (times the 1e4 values) dominate
# dqkv and dtable: no fp32 evaluation can be compared there.  With the 2400 query rows of the 2 x 3 grid (B 2, nH 2)
# every seed tried has such rows at ws 10 (the fp64 reference itself moves by 1e-3 when the inputs move by half an fp32
# ulp, and max |dqkv| passes the fp16 range); the 36 or 100 rows of one window do not.
# tests/test_window_attn_sweep_cpu.py asserts the condition, on the reference alone.
TAIL_CASES = [c for c in CASES if c.group == "few" and c.ws in (6, 10) and c.windows == (1, 1)]


def tail_inputs(c, dtype):
    qkv, table, gout = make_inputs(c)
    return fill_last_tokens(c, qkv).to(dtype), table.float(), gout.to(dtype)


def reference(c, qkv, table, gout, fn=window_attention_ref, shift=None, scale=None):
    """fp64 out, dqkv, dtable of ``fn`` on the values the given tensors hold (so a 16-bit run is measured against the
    exact result for its rounded inputs)."""
    q = qkv.detach().double().requires_grad_()
    t = table.detach().double().requires_grad_()
    out = fn(q, t, c.nH, c.ws, c.shift if shift is None else shift, scale_of(c) if scale is None else scale)
    out.backward(gout.detach().double())
    return out.detach(), q.grad, t.grad
