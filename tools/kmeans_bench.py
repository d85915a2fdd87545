#!/usr/bin/env python3
"""One Lloyd iteration over scene latents: `eae_kmeans_assign` + `eae_kmeans_update` (two passes over z, no N x K matrix, centroids
bitwise repeatable) against the torch route on the same tensors (`cdist` -> `argmin` -> `index_add_` / `bincount`: an N x K matrix,
a float-atomic scatter).  N = 2^20 rows (an 8192^2 scene at stride 8), L = 64, K in {10, 64, 256}.

The two routes' labels are compared first (they may differ on fp32 near-ties only: the share is printed).  Then the arms alternate
inside one process after --warmup rounds; a repetition is --iters iterations between device events, ending in a synchronise; median,
min and max per iteration over --reps.  assign and update are also timed alone.  Peak extra memory is
`torch.cuda.max_memory_allocated` over one iteration less what was allocated before it (the kernels' workspace included).  The
floors printed with each shape are computed from the shapes: one read of z per pass at 6.3 TB/s, and 2 N K L FLOP per pass at the
122 TFLOP/s an untuned f32-input MFMA GEMM reaches.

    python tools/kmeans_bench.py [--reps 7] [--warmup 2] [--iters 5] [--rows 1048576]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd import cluster  # noqa: E402

L = 64
HBM_BPS, MFMA_F32_FLOPS = 6.3e12, 122e12


def torch_iteration(z, cent):
    k = cent.shape[0]
    labels = torch.cdist(z, cent).argmin(1)
    sums = torch.zeros_like(cent).index_add_(0, labels, z)
    counts = torch.bincount(labels, minlength=k)
    return torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], cent), labels


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


def bench(n, k, reps, warmup, iters):
    g = torch.Generator().manual_seed(k)
    # latents with structure: k blobs of unit spread around centres of norm 4, so that clusters have members
    centres = torch.randn((k, L), generator=g)
    centres *= 4.0 / centres.norm(dim=1, keepdim=True)
    z = (centres[torch.randint(0, k, (n,), generator=g)] + torch.randn((n, L), generator=g)).cuda()
    cent0 = eae_amd.kmeans_init(z, k, seed=0)
    labels = torch.empty(n, dtype=torch.int64, device="cuda")
    dist = torch.empty(n, dtype=torch.float32, device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    cent = cent0.clone()

    def ours_alloc():                       # what a caller pays in memory: outputs aside, the update's workspace
        ws = cluster._workspace(z, k)
        cluster._assign(z, cent, labels, dist)
        cluster._update(z, labels, cent, counts, ws)
        return ws

    ws = cluster._workspace(z, k)
    arms = {"kmeans_kernels": lambda: (cluster._assign(z, cent, labels, dist), cluster._update(z, labels, cent, counts, ws)),
            "torch_cdist_index_add": lambda: torch_iteration(z, cent0),
            "assign_only": lambda: cluster._assign(z, cent0, labels, dist),
            "update_only": lambda: cluster._update(z, labels, cent, counts, ws)}
    cluster._assign(z, cent0, labels, dist)
    differ = int((labels != torch_iteration(z, cent0)[1]).sum())
    peak = {"kmeans_kernels": _peak_extra(ours_alloc), "torch_cdist_index_add": _peak_extra(arms["torch_cdist_index_add"])}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():                        # alternating
            ts[name].append(_timed(fn, iters))
    zbytes, flop = n * L * 4, 2.0 * n * k * L
    res = {"bench": "kmeans", "rows": n, "latent": L, "k": k, "reps": reps, "iters_per_rep": iters, "labels_differing_from_torch": differ,
           "floor_ms_per_pass": {"hbm_read_of_z": round(zbytes / HBM_BPS * 1e3, 4), "f32_mfma": round(flop / MFMA_F32_FLOPS * 1e3, 4)}}
    for name, v in ts.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
        if name in peak:
            res[name]["peak_extra_bytes"] = peak[name]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a GPU: nothing is measured without one")
    for k in (10, 64, 256):
        print(json.dumps(bench(a.rows, k, a.reps, a.warmup, a.iters)), flush=True)


if __name__ == "__main__":
    main()
