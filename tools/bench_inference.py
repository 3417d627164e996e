"""Time the fused inference heads against a straight torch restatement of the reference's eval branch
(maskformer_model.py:337-377 + :509-624) on the same GPU, in the same run.

    python tools/bench_inference.py [--size 1024] [--reps 20] [--out profiles/inference_heads.json]

One image, Q = 100, K = 133 (things 0..79), padded/image/output size --size squared, logits at a quarter of it, in
fp32 and fp16.  Each entry is milliseconds per image between two device events around `reps` calls after warm-up, so
it includes the Python glue and, for the panoptic head, its one device-to-host copy (the torch baseline's includes
its 3 x n_keep `.item()` calls).  Bytes and FLOPs are the algorithmic counts of the fused heads (logits read once,
result written once; 2 K Q H W for the semantic contraction); `frac_of_bound` is the larger of bytes / measured HBM
rate and FLOPs / measured f32-MFMA rate over the measured time, with both rates probed in this run (the stream copy
bench.py --full uses, and the library's own f32-MFMA GEMM).  Needs a HIP device; there is no CPU mode.  Prints one
JSON line.

`instance` times the instance head alone (with the thing filter, as the baseline); `semantic_full_res` times the
compat function `semantic_inference` on masks already at full resolution against the baseline's einsum on the same
tensor (no upsample on either side).  Both versions of a head get two windows of `reps` calls, alternated, and the
faster window of each is reported."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bm2f_amd import MaskFormerInference, _native, semantic_inference  # noqa: E402
from bm2f_amd.inference import _finish_instances, _instance_hip  # noqa: E402

Q, K, THINGS, TOPK = 100, 133, 80, 100
OBJ_THR = OVL_THR = 0.8


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def make_inputs(size, device):
    g = torch.Generator().manual_seed(0)
    cls = torch.randn(1, Q, K + 1, generator=g) * 0.1
    cls[..., K] += 10
    kept = torch.randperm(Q, generator=g)[:12]
    for q in kept:                                  # a dozen confident queries, the rest void
        cls[0, q, K] -= 10
        cls[0, q, int(torch.randint(0, K, (1,), generator=g))] += 12
    masks = torch.randn(1, Q, size // 4, size // 4, generator=g) * 3
    return cls.to(device), masks.to(device)


# ---- the torch baseline: the reference's eval branch restated -------------------------------------------------------
def torch_upsample(masks, size):
    return F.interpolate(masks, size=(size, size), mode="bilinear", align_corners=False)[0]


def torch_semantic(cls, up):
    return torch.einsum("qc,qhw->chw", F.softmax(cls, dim=-1)[..., :-1], up.sigmoid())


def torch_panoptic(cls, up):
    scores, labels = F.softmax(cls, dim=-1).max(-1)
    mask_pred = up.sigmoid()
    keep = labels.ne(K) & (scores > OBJ_THR)
    cur_scores, cur_classes, cur_masks = scores[keep], labels[keep], mask_pred[keep]
    cur_prob_masks = cur_scores.view(-1, 1, 1) * cur_masks
    panoptic_seg = torch.zeros(cur_masks.shape[-2:], dtype=torch.int32, device=cur_masks.device)
    info, cur, memory = [], 0, {}
    if cur_masks.shape[0] == 0:
        return panoptic_seg, info
    ids = cur_prob_masks.argmax(0)
    for k in range(cur_classes.shape[0]):
        pc = cur_classes[k].item()
        isthing = pc < THINGS
        mask_area = (ids == k).sum().item()
        original_area = (cur_masks[k] >= 0.5).sum().item()
        mask = (ids == k) & (cur_masks[k] >= 0.5)
        if mask_area > 0 and original_area > 0 and mask.sum().item() > 0:
            if mask_area / original_area < OVL_THR:
                continue
            if not isthing:
                if pc in memory:
                    panoptic_seg[mask] = memory[pc]
                    continue
                memory[pc] = cur + 1
            cur += 1
            panoptic_seg[mask] = cur
            info.append({"id": cur, "isthing": isthing, "category_id": pc})
    return panoptic_seg, info


def torch_instance(cls, up):
    scores = F.softmax(cls, dim=-1)[:, :-1]
    s, idx = scores.flatten(0, 1).topk(TOPK, sorted=False)
    lab = idx % K
    m = up[idx // K]
    keep = lab < THINGS
    s, lab, m = s[keep], lab[keep], m[keep]
    binary = (m > 0).float()
    ms = (m.sigmoid().flatten(1) * binary.flatten(1)).sum(1) / (binary.flatten(1).sum(1) + 1e-6)
    return binary, s * ms, lab


def probes(device):
    st = torch.cuda.current_stream(device).cuda_stream
    nbytes = 1 << 30
    a = torch.empty(nbytes, dtype=torch.uint8, device=device).fill_(1)
    b = torch.empty_like(a)
    t_copy = min(timed(lambda: _native.call("m2f_stream_copy", a.data_ptr(), b.data_ptr(), nbytes, mode, st), 10)
                 for mode in (0, 1))
    del a, b
    m, n, k = 16384, 1024, 1024
    x, w = torch.randn(m, k, device=device), torch.randn(n, k, device=device)
    out = torch.empty(m, n, device=device)
    t_mm = timed(lambda: _native.call("m2f_gemm_f32_nt", x.data_ptr(), k, w.data_ptr(), k, None, 0, None, 0,
                                      out.data_ptr(), n, m, n, k, st), 20)
    del x, w, out
    torch.cuda.empty_cache()
    return {"hbm_gbs": round(2 * nbytes / (t_copy * 1e-3) / 1e9, 1),
            "f32_mfma_tflops": round(2 * m * n * k / (t_mm * 1e-3) / 1e12, 1),
            "hbm_probe": "m2f_stream_copy, 1 GiB in + 1 GiB out, mean of 10, the faster of its two modes",
            "f32_mfma_probe": f"m2f_gemm_f32_nt {m}x{n}x{k}, mean of 20"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference: needs a HIP device")
    dev = torch.device("cuda:0")
    size, sizes = a.size, [(a.size, a.size)]
    peaks = probes(dev)
    px, logit_elems = size * size, Q * (size // 4) ** 2
    common = dict(num_classes=K, thing_classes=range(THINGS), object_mask_threshold=OBJ_THR,
                  overlap_threshold=OVL_THR, test_topk_per_image=TOPK, sem_seg_postprocess_before_inference=True)
    heads = {"semantic": MaskFormerInference(semantic_on=True, **common),
             "panoptic": MaskFormerInference(semantic_on=False, panoptic_on=True, **common)}
    res = {"bench": "inference_heads", "device": torch.cuda.get_device_name(0), "size": size, "Q": Q, "K": K,
           "logits": [size // 4, size // 4], "reps": a.reps, "peaks": peaks, "results": {}}
    for dt_name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
        cls, masks = make_inputs(size, dev)
        out = {"pred_logits": cls, "pred_masks": masks.to(dt)}
        lb = logit_elems * out["pred_masks"].element_size()
        n_sel = int(torch.unique(F.softmax(cls[0], -1)[:, :-1].flatten().topk(TOPK).indices // K).numel())
        counts = {"semantic": (lb + K * px * 4, 2 * K * Q * px), "semantic_labels": (lb + px * 2, 2 * K * Q * px),
                  "panoptic": (lb + px * 3 + px * 4, 0), "instance": (lb + n_sel * px, 0),
                  "semantic_full_res": (Q * px * out["pred_masks"].element_size() + K * px * 4, 2 * K * Q * px)}
        geo = [(size, size, size, size)]
        up_in = torch_upsample(out["pred_masks"], size)   # the compat functions' input: masks already upsampled
        fused = {"semantic": lambda: heads["semantic"](out, sizes[0], sizes, sizes),
                 "semantic_labels": lambda: heads["semantic"](out, sizes[0], sizes, sizes, semantic_labels=True),
                 "panoptic": lambda: heads["panoptic"](out, sizes[0], sizes, sizes),
                 # the instance head alone, with the thing filter of the panoptic setting (as torch_instance)
                 "instance": lambda: [_finish_instances(r, None) for r in _instance_hip(
                     cls, out["pred_masks"], sizes[0], geo, K, TOPK, range(THINGS))],
                 "semantic_full_res": lambda: semantic_inference(cls[0], up_in)}
        # the baseline runs the reference's way: upsample once per image, then the head (in the logits' dtype)
        m_in = out["pred_masks"]
        c_in = cls[0].to(dt)
        base = {"upsample": lambda: torch_upsample(m_in, size),
                "semantic": lambda: torch_semantic(c_in, torch_upsample(m_in, size)),
                "semantic_labels": lambda: torch_semantic(c_in, torch_upsample(m_in, size)).argmax(0),
                "panoptic": lambda: torch_panoptic(c_in, torch_upsample(m_in, size)),
                "instance": lambda: torch_instance(c_in, torch_upsample(m_in, size)),
                "semantic_full_res": lambda: torch_semantic(c_in, up_in)}
        entry = {"torch_upsample_ms": round(timed(base["upsample"], a.reps), 4)}
        for name in ("semantic", "semantic_labels", "panoptic", "instance", "semantic_full_res"):
            # alternate the two versions, two windows of the same length each; report the faster window of each
            t1 = timed(fused[name], a.reps)
            b1 = timed(base[name], a.reps)
            t2 = timed(fused[name], a.reps)
            b2 = timed(base[name], a.reps)
            t, tb = min(t1, t2), min(b1, b2)
            nbytes, flops = counts[name]
            bound_s = max(nbytes / (peaks["hbm_gbs"] * 1e9), flops / (peaks["f32_mfma_tflops"] * 1e12))
            entry[name] = {"fused_ms": round(t, 4), "fused_ms_windows": [round(t1, 4), round(t2, 4)],
                           "torch_ms": round(tb, 4), "torch_ms_windows": [round(b1, 4), round(b2, 4)], "speedup": round(tb / t, 2), "bytes": nbytes, "flops": flops,
                           "bound": "mfma" if flops / (peaks["f32_mfma_tflops"] * 1e12) * 1e3 >= nbytes /
                           (peaks["hbm_gbs"] * 1e9) * 1e3 else "hbm",
                           "frac_of_bound": round(bound_s * 1e3 / t, 3)}
        res["results"][dt_name] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
