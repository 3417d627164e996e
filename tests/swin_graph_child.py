"""Child process of ``test_swin_gpu.test_graph_capture_no_memset``: forward + backward of window_attention (op case
b of tests/golden) captured with ``torch.cuda.graph`` in a fresh process.  The captured graph must hold no memset node
(a captured memset replays wrongly under the runtime's graph packet capture) and every replay must equal the eager
result bit for bit.  Prints ``SWIN_GRAPH_OK`` and exits 0 on success.

    python tests/swin_graph_child.py [--dtype fp16|fp32] [--replays 3]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--replays", type=int, default=3)
    a = ap.parse_args()
    import torch

    from bm2f_amd import window_attention
    from bm2f_amd.bench_model import graph_node_counts
    from swin_ref import load_golden
    dev = torch.device("cuda:0")
    dt = {"fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    fx = load_golden("swin_op_b")
    _, nH, _, _, ws, shift = (int(v) for v in fx["meta"])
    gout = torch.from_numpy(fx["gout"]).to(dev, dt)

    def leaves():
        return (torch.from_numpy(fx["qkv"]).to(dev, dt).requires_grad_(),
                torch.from_numpy(fx["table"]).to(dev).requires_grad_())

    def run(qkv, table):
        out = window_attention(qkv, table, nH, ws, shift)
        dq, dtab = torch.autograd.grad(out, (qkv, table), gout)
        return out.detach(), dq, dtab

    # the eager copy runs on leaves of its own and keeps no autograd graph: a graph kept alive from a run on the
    # default stream would tie the captured backward to that stream
    eager = [t.clone() for t in run(*leaves())]
    qkv, table = leaves()

    def step():
        return run(qkv, table)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        res = step()
    nodes = graph_node_counts(graph)
    print(f"captured nodes: {nodes}", flush=True)
    if nodes.get("memset"):
        print("FAIL: memset node in the captured step", flush=True)
        return 1
    if not nodes.get("kernel"):
        print("FAIL: no kernel node captured", flush=True)
        return 1
    graph.instantiate()
    bad = 0
    for i in range(a.replays):
        for t in res:
            t.fill_(float("nan"))     # a replay that skipped a kernel would leave these
        graph.replay()
        torch.cuda.synchronize()
        same = [torch.equal(g, e) for g, e in zip(res, eager)]
        print(f"replay {i + 1}: out/dqkv/dtable equal eager: {same}", flush=True)
        bad += sum(not s for s in same)
    if bad:
        print("FAIL", flush=True)
        return 1
    print("SWIN_GRAPH_OK", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
