#!/usr/bin/env python3
"""The Gaussian classifier's two kernels against the torch routes on the same tensors.

- `gaussian_predict` (`eae_gauss_score`: one launch, no N x K x L temporary) against a chunked torch baseline: for every chunk of
  --chunk rows and every class ``((z - mu_k) @ W_k).square().sum(1) + offset_k`` into a [chunk, K] matrix, then ``argmin``.
- `class_scatter` (a stable sort, `eae_kmeans_update` for the means, `eae_class_scatter`) against per-class ``d.T @ d`` over
  boolean-indexed rows, d = z[labels == k] - mean_k.

Shapes (N, L, K): (2^20, 64, 10), (2^20, 64, 64), (2^17, 256, 10).  Every shape runs in a child process of its own under
`timeout`; the first child that fails ends the run.  Inside a child the arms alternate after --warmup rounds; a repetition is --iters
calls between device events, ending in a synchronise; median, min and max per call over --reps.  Peak extra memory is
`torch.cuda.max_memory_allocated` over one call less what was allocated before it (outputs and workspaces included).  The score
kernel's share of the f32-input MFMA rate is 2 N K L^2 FLOP over its time over 155 TFLOP/s.  The labels of the two predict routes
are compared first (they may differ on fp32 near-ties only: the number is printed), and the two scatters by their largest difference
relative to the largest element.

    python tools/gaussian_bench.py [--reps 7] [--warmup 2] [--iters 5] [--chunk 131072] [--limit 240]   ->  JSON lines
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1 << 20, 64, 10), (1 << 20, 64, 64), (1 << 17, 256, 10)]
MFMA_F32_FLOPS = 155e12


def torch_predict(z, model, chunk):
    k = model.means.shape[0]
    labels = torch.empty(z.shape[0], dtype=torch.int64, device=z.device)
    maha = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
    for lo in range(0, z.shape[0], chunk):
        zc = z[lo:lo + chunk]
        d = torch.empty((zc.shape[0], k), dtype=torch.float32, device=z.device)
        for q in range(k):
            d[:, q] = ((zc - model.means[q]) @ model.whiten[q if model.whiten.shape[0] > 1 else 0]).square().sum(1)
        lab = (d + model.offset).argmin(1)
        labels[lo:lo + chunk] = lab
        maha[lo:lo + chunk] = d.gather(1, lab[:, None])[:, 0]
    return labels, maha


def torch_scatter(z, labels, k):
    out = torch.zeros((k, z.shape[1], z.shape[1]), dtype=torch.float32, device=z.device)
    for q in range(k):
        rows = z[labels == q]
        if rows.shape[0]:
            d = rows - rows.mean(0)
            out[q] = d.T @ d
    return out


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def bench(n, width, k, reps, warmup, iters, chunk):
    import eae_amd
    g = torch.Generator().manual_seed(k + width)
    # latents with structure: k blobs of unit spread around centres of norm 4, a mixing matrix of its own each
    centres = torch.randn((k, width), generator=g)
    centres *= 4.0 / centres.norm(dim=1, keepdim=True)
    ids = torch.randint(0, k, (n,), generator=g)
    z = (centres[ids] + torch.randn((n, width), generator=g) / width ** 0.5).cuda()
    ids = ids.cuda()
    model = eae_amd.gaussian_fit(z, ids, k)
    arms = {"gaussian_predict": lambda: eae_amd.gaussian_predict(z, model),
            "torch_predict_chunked": lambda: torch_predict(z, model, chunk),
            "class_scatter": lambda: eae_amd.class_scatter(z, ids, k),
            "torch_scatter_per_class": lambda: torch_scatter(z, ids, k)}
    differ = int((arms["gaussian_predict"]()[0] != arms["torch_predict_chunked"]()[0]).sum())
    ours, theirs = arms["class_scatter"]()[2], arms["torch_scatter_per_class"]()
    scatter_diff = float((ours - theirs).abs().max() / theirs.abs().max())
    peak = {name: _peak_extra(fn) for name, fn in arms.items()}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():                        # alternating
            ts[name].append(_timed(fn, iters))
    flop = 2.0 * n * k * width * width
    res = {"bench": "gaussian", "rows": n, "latent": width, "k": k, "reps": reps, "iters_per_rep": iters, "torch_chunk_rows": chunk,
           "labels_differing_from_torch": differ, "scatter_max_rel_diff_from_torch": scatter_diff,
           "score_gflop": round(flop / 1e9, 2)}
    for name, v in ts.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "peak_extra_bytes": peak[name]}
    res["gaussian_predict"]["share_of_155_tflops_f32_mfma"] = round(flop / (res["gaussian_predict"]["ms"] * 1e-3) / MFMA_F32_FLOPS, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(internal) run this shape in this process")
    a = ap.parse_args()
    if a.shape is not None:
        if not torch.cuda.is_available():
            raise SystemExit("gaussian_bench needs a GPU: nothing is measured without one")
        print(json.dumps(bench(*SHAPES[a.shape], a.reps, a.warmup, a.iters, a.chunk)), flush=True)
        return
    for i in range(len(SHAPES)):                             # a fresh process and a time limit for every shape; stop at the first failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--shape", str(i), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--iters", str(a.iters), "--chunk", str(a.chunk)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"shape {SHAPES[i]} ended with status {rc}: nothing further is run")


if __name__ == "__main__":
    main()
