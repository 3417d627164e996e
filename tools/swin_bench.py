"""Time the fused shifted-window attention against the torch path of the same definition, forward + backward, at the
Swin stage shapes of the benchmarked configs; writes profiles/swin_window_attention.json.

    python tools/swin_bench.py [--rounds 3] [--window 0.25] [--out profiles/swin_window_attention.json]

Shapes: the four Swin-L stages at 1024 x 1024 (C 192/384/768/1536, heads 6/12/24/48, ws 12, grids 256/128/64/32 squared,
padded to a multiple of 12, 2 images per rank as config 4) and Swin-T's first stage of config 5 (C 96, 3 heads, ws 7,
10 frames of 384 x 640 -> grid 96 x 160).  Two levels: the op alone, and one SwinTransformerBlock (shifted).  The
baseline is the torch path (roll, partition, matmul, softmax, reverse) on the same device in the same process; the two
sides are timed in alternating rounds and the median round is reported, with the peak memory of one fwd + bwd.  Each
timed window runs as many iterations as fill ``--window`` seconds of device time (counted from a short calibration run
and recorded per entry), so that a window is never a few milliseconds of work.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # name, batch, C, heads, ws, H, W
    ("swin_l_stage1", 2, 192, 6, 12, 256, 256),
    ("swin_l_stage2", 2, 384, 12, 12, 128, 128),
    ("swin_l_stage3", 2, 768, 24, 12, 64, 64),
    ("swin_l_stage4", 2, 1536, 48, 12, 32, 32),
    ("swin_t_stage1_video", 10, 96, 3, 7, 96, 160),
]


def timed(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    return run_timed(fn, iters)


def run_timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def iters_for(fn, window_s):
    """Iterations that fill `window_s` seconds, from a calibration of a few iterations after warm-up."""
    ms = timed(fn, 5)
    return max(5, int(window_s * 1e3 / ms) + 1)


def compare(kernel, torch_path, rounds, window_s):
    nk, nt = iters_for(kernel, window_s), iters_for(torch_path, window_s)
    tk, tt = [], []
    for _ in range(rounds):
        tk.append(timed(kernel, nk))
        tt.append(timed(torch_path, nt))
    k, t = statistics.median(tk), statistics.median(tt)
    return {"kernel_ms": round(k, 4), "torch_ms": round(t, 4), "torch_over_kernel": round(t / k, 3),
            "kernel_iters": nk, "torch_iters": nt,
            "kernel_ms_rounds": [round(v, 4) for v in tk], "torch_ms_rounds": [round(v, 4) for v in tt],
            "kernel_peak_mib": round(peak(kernel), 1), "torch_peak_mib": round(peak(torch_path), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--out", default=os.path.join("profiles", "swin_window_attention.json"))
    a = ap.parse_args()
    import torch

    from bm2f_amd import swin
    dev = torch.device("cuda:0")
    real = swin.window_attention

    def torch_op(q, t, nH, ws, shift, scale=None):
        return swin.window_attention_torch(q, t, nH, ws, shift, scale)

    results = []
    for name, B, C, nH, ws, H, W in SHAPES:
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        for dname, dt in (("fp16", torch.float16), ("fp32", torch.float32)):
            torch.manual_seed(0)
            qkv = torch.randn(B, Hp, Wp, 3 * C, device=dev, dtype=dt, requires_grad=True)
            table = torch.randn((2 * ws - 1) ** 2, nH, device=dev, requires_grad=True)
            gout = torch.randn(B, Hp, Wp, C, device=dev, dtype=dt)

            def op(fn):
                def run():
                    out = fn(qkv, table, nH, ws, ws // 2)
                    torch.autograd.grad(out, (qkv, table), gout)
                return run

            row = {"shape": name, "dtype": dname, "batch": B, "channels": C, "heads": nH, "window": ws,
                   "grid": [H, W], "padded_grid": [Hp, Wp], "shift": ws // 2}
            row["op"] = compare(op(real), op(torch_op), a.rounds, a.window)
            del qkv, gout

            blk = swin.SwinTransformerBlock(dim=C, num_heads=nH, window_size=ws, shift_size=ws // 2).to(dev)
            blk.H, blk.W = H, W
            x = torch.randn(B, H * W, C, device=dev, requires_grad=True)
            gy = torch.randn(B, H * W, C, device=dev)

            def block(fn):
                def run():
                    swin.window_attention = fn
                    try:
                        with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=dt == torch.float16):
                            y = blk(x)
                        torch.autograd.grad(y, [x, *blk.parameters()], gy)
                    finally:
                        swin.window_attention = real
                return run

            row["block"] = compare(block(real), block(torch_op), a.rounds, a.window)
            del blk, x, gy
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            results.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window,
           "note": "fwd + bwd, median of alternating rounds; torch = the torch path of the same definition",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
