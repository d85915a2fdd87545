#!/usr/bin/env python3
"""Nearest-neighbour search over scene latents: `knn_search` (`eae_knn_search`: the bank streams through the kernel, each query's k best
stay on chip, no Nq x M matrix, exact tie order) against the torch route on the same tensors (`cdist` -> `topk`, over chunks of
--chunk-mib of distance matrix at a time, because the whole matrix of the first shape is 32 GiB).  L = 64, k = 10, two shapes:
    Nq = 2^20, M = 8192     a scene's windows (8192^2 at stride 8) against a labelled bank
    Nq = 16,   M = 2^20     retrieval: a handful of examples against a scene's windows (the bank is cut into slices)

The two routes' neighbour lists are compared first (they may differ on fp32 near-ties only: the share of rows is printed).  Then the
arms alternate inside one process after --warmup rounds; a repetition is --iters calls between device events, ending in a
synchronise; median, min and max per call over --reps.  Peak extra memory is `torch.cuda.max_memory_allocated` over one call less what
was allocated before it (outputs and the kernel's workspace included).  The floors printed with each shape are computed from the
shapes: one read of the queries and the bank at 6.3 TB/s, and 2 Nq M L FLOP at the 157.3 TFLOP/s peak of the f32-input MFMA.

    python tools/knn_bench.py [--reps 7] [--warmup 2] [--iters 3] [--chunk-mib 256]   ->  JSON lines
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

L, K = 64, 10
HBM_BPS, MFMA_F32_FLOPS = 6.3e12, 157.3e12
SHAPES = [(1 << 20, 8192), (16, 1 << 20)]


def torch_knn(q, bank, k, chunk_rows):
    idx = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    dist = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    for lo in range(0, q.shape[0], chunk_rows):
        d, i = torch.cdist(q[lo:lo + chunk_rows], bank).topk(k, dim=1, largest=False)
        idx[lo:lo + chunk_rows], dist[lo:lo + chunk_rows] = i, d * d
    return idx, dist


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


def bench(nq, m, reps, warmup, iters, chunk_mib):
    g = torch.Generator().manual_seed(nq % 1000 + m % 1000)
    # latents with structure: blobs of unit spread around 10 centres of norm 4, as the k-means bench draws them
    centres = torch.randn((10, L), generator=g)
    centres *= 4.0 / centres.norm(dim=1, keepdim=True)
    q = (centres[torch.randint(0, 10, (nq,), generator=g)] + torch.randn((nq, L), generator=g)).cuda()
    bank = (centres[torch.randint(0, 10, (m,), generator=g)] + torch.randn((m, L), generator=g)).cuda()
    chunk_rows = max(1, min(nq, (chunk_mib << 20) // (4 * m)))
    arms = {"knn_search": lambda: eae_amd.knn_search(q, bank, K),
            "torch_cdist_topk": lambda: torch_knn(q, bank, K, chunk_rows)}
    ours, ref = arms["knn_search"](), arms["torch_cdist_topk"]()
    differ = int((ours.idx != ref[0]).any(dim=1).sum())
    peak = {name: _peak_extra(fn) for name, fn in arms.items()}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():                        # alternating
            ts[name].append(_timed(fn, iters))
    lib = _lib.load()
    res = {"bench": "knn", "queries": nq, "bank": m, "latent": L, "k": K, "reps": reps, "iters_per_rep": iters,
           "bank_slices": lib.eae_knn_slices(nq, m, L, K), "workspace_bytes": lib.eae_knn_workspace_bytes(nq, m, L, K),
           "torch_chunk_rows": chunk_rows, "rows_differing_from_torch": differ,
           "floor_ms": {"hbm_read_of_q_and_bank": round((nq + m) * L * 4 / HBM_BPS * 1e3, 4),
                        "f32_mfma": round(2.0 * nq * m * L / MFMA_F32_FLOPS * 1e3, 4)}}
    for name, v in ts.items():
        v.sort()
        res[name] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "peak_extra_bytes": peak[name]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunk-mib", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU: nothing is measured without one")
    for nq, m in SHAPES:
        print(json.dumps(bench(nq, m, a.reps, a.warmup, a.iters, a.chunk_mib)), flush=True)


if __name__ == "__main__":
    main()
