#!/usr/bin/env python3
"""Confusion counts of a cell map against a label raster: `scene_confusion` (one kernel reading the raster and the mask once)
against the torch route (upsample the cell map with two `repeat_interleave`s, crop, form truth * (K + 1) + pred, `bincount`).
8192 x 8192 uint8 truth, K = 10, cells of 16, with and without a mask.

The two count matrices are asserted equal first.  Then the arms alternate inside one process after --warmup rounds; a repetition
is one call between device events, ending in a synchronise; median, min and max of --reps.  TB/s counts the truth and mask bytes,
the bytes the algorithm has to read.  Each arm's peak extra allocation is `torch.cuda.max_memory_allocated` over one call less what
was allocated before it.  The kernel alone comes from a separate `rocprofv3 --kernel-trace --stats -- python
tools/scene_confusion_bench.py` run (scene_confusion_kernel).

    python tools/scene_confusion_bench.py [--reps 7] [--warmup 2] [--size 8192]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402

K, CELL = 10, 16


def torch_route(pred, truth, mask):
    h, w = truth.shape
    up = pred.repeat_interleave(CELL, 0).repeat_interleave(CELL, 1)[:h, :w]
    c = torch.where((up >= 0) & (up < K), up, K)
    t = truth.to(torch.int64)
    idx = torch.where(t < K, t, K) * (K + 1) + c
    if mask is not None:
        idx = idx[mask == 0]
    return torch.bincount(idx.reshape(-1), minlength=(K + 1) ** 2).reshape(K + 1, K + 1)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def bench(size, masked, reps, warmup):
    g = torch.Generator().manual_seed(size + masked)
    # a land-cover-like raster: 32 x 32 blocks of one class, 10 % single-pixel noise, 255 = unlabelled
    coarse = torch.randint(0, K + 1, (size // 32, size // 32), generator=g)
    truth = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)
    noise = torch.rand((size, size), generator=g) < 0.1
    truth = torch.where(noise, torch.randint(0, K + 1, (size, size), generator=g), truth)
    truth = torch.where(truth == K, 255, truth).to(torch.uint8).cuda()
    pred = torch.randint(-1, K, (size // CELL, size // CELL), generator=g).cuda()
    mask = (torch.rand((size, size), generator=g) < 0.25).cuda() if masked else None
    arms = {"scene_confusion": lambda: eae_amd.scene_confusion(pred, truth, K, cell=CELL, mask=mask),
            "torch_bincount": lambda: torch_route(pred, truth, mask)}
    a, b = (fn() for fn in arms.values())
    assert torch.equal(a, b), "the two routes disagree"
    assert int(a.sum()) == size * size - (int(mask.sum()) if masked else 0)
    del a, b
    peak = {k: _peak_extra(fn) for k, fn in arms.items()}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():                           # alternating
            ts[k].append(_timed(fn))
    nbytes = size * size * (2 if masked else 1)
    res = {"bench": "scene_confusion", "truth": [size, size], "dtype": "uint8", "classes": K, "cell": CELL, "mask": bool(masked),
           "reps": reps, "bytes": nbytes}
    for k, v in ts.items():
        v.sort()
        med = v[len(v) // 2]
        res[k] = {"ms": round(med, 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                  "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "peak_extra_bytes": peak[k]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_confusion_bench needs a GPU: nothing is measured without one")
    for masked in (0, 1):
        print(json.dumps(bench(a.size, masked, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
