#!/usr/bin/env python3
"""The silhouette coefficient of latents: `silhouette_score` (`eae_class_dist_sums`: the bank streams through the kernel class by class,
every query's distances are added on chip, no N x N matrix) against the torch route on the same tensors (`cdist(chunk, z) @ onehot`
over chunks of --chunk-mib of distance matrix at a time, because the whole matrix of the last shape's bank would be 4 TiB).  L = 64,
labels uniform over K classes of blobs of unit spread:
    N = 2^17, K = 10         every row against every row
    N = 2^17, K = 256        the same with many short segments
    N = 2^20, K = 10, sample = 8192      8192 drawn rows against all rows

The two routes' scores are compared first.  Then the arms alternate inside one process after --warmup rounds; a repetition is --iters
calls between device events, ending in a synchronise; median, min and max per call over --reps.  Peak extra memory is
`torch.cuda.max_memory_allocated` over one call less what was allocated before it (the sorted copy of the bank, the sums and the
kernel's workspace included).  The floor printed with each shape is 2 Nq N L FLOP at the 157.3 TFLOP/s peak of the f32-input MFMA.

    python tools/silhouette_bench.py [--reps 5] [--warmup 1] [--iters 2] [--chunk-mib 256]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd import _lib  # noqa: E402

L = 64
MFMA_F32_FLOPS = 157.3e12
SHAPES = [(1 << 17, 10, None), (1 << 17, 256, None), (1 << 20, 10, 8192)]


def torch_silhouette(z, labels, k, rows, chunk_rows):
    """The mean silhouette by `cdist` and a one-hot product, a chunk of query rows at a time (a row's distance to itself is 0, so
    nothing has to be left out of its own class's sum)."""
    onehot = torch.nn.functional.one_hot(labels, k).to(torch.float32)
    counts = onehot.sum(0).to(torch.float64)
    q = z if rows is None else z[rows]
    qlab = labels if rows is None else labels[rows]
    sums = torch.empty((q.shape[0], k), dtype=torch.float32, device=z.device)
    for lo in range(0, q.shape[0], chunk_rows):
        sums[lo:lo + chunk_rows] = torch.cdist(q[lo:lo + chunk_rows], z) @ onehot
    sums = sums.to(torch.float64)
    a = sums.gather(1, qlab[:, None]).squeeze(1) / (counts[qlab] - 1).clamp(min=1)
    b = (sums / counts[None, :]).scatter(1, qlab[:, None], float("inf")).min(dim=1).values
    return ((b - a) / torch.maximum(a, b)).mean()


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


def bench(n, k, sample, reps, warmup, iters, chunk_mib):
    g = torch.Generator().manual_seed(n % 1000 + k)
    centres = torch.randn((k, L), generator=g)
    centres *= 4.0 / centres.norm(dim=1, keepdim=True)
    labels = torch.randint(0, k, (n,), generator=g)
    z = (centres[labels] + torch.randn((n, L), generator=g)).cuda()
    labels = labels.cuda()
    rows = None if sample is None else torch.randperm(n, generator=torch.Generator().manual_seed(0))[:sample].cuda()
    nq = n if sample is None else sample
    chunk_rows = max(1, min(nq, (chunk_mib << 20) // (4 * n)))
    arms = {"silhouette_score": lambda: eae_amd.silhouette_score(z, labels, k, sample=sample, seed=0)[0],
            "torch_cdist_onehot": lambda: torch_silhouette(z, labels, k, rows, chunk_rows)}
    ours, ref = float(arms["silhouette_score"]()), float(arms["torch_cdist_onehot"]())
    peak = {name: _peak_extra(fn) for name, fn in arms.items()}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():                        # alternating
            ts[name].append(_timed(fn, iters))
    res = {"bench": "silhouette", "rows": n, "queries": nq, "latent": L, "classes": k, "reps": reps, "iters_per_rep": iters,
           "workspace_bytes": _lib.load().eae_class_dist_workspace_bytes(nq, n, L, k), "torch_chunk_rows": chunk_rows,
           "score": ours, "score_torch": ref, "floor_ms": {"f32_mfma": round(2.0 * nq * n * L / MFMA_F32_FLOPS * 1e3, 4)}}
    for name, v in ts.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "peak_extra_bytes": peak[name]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--chunk-mib", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench needs a GPU: nothing is measured without one")
    for n, k, sample in SHAPES:
        print(json.dumps(bench(n, k, sample, a.reps, a.warmup, a.iters, a.chunk_mib)), flush=True)


if __name__ == "__main__":
    main()
