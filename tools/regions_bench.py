#!/usr/bin/env python3
"""Map post-processing on the device: ms and peak extra device memory of `label_regions`, `majority_filter(radius=2)` and
`sieve(min_size=16)` on 4096 x 4096 int64 maps:

  upsampled    ten classes, a 512 x 512 random map upsampled 8 x by nearest neighbour: what a cell map looks like
  percolation  two classes at p = 0.59, near the percolation threshold: large, tortuous regions
  serpentine   a 1-wide path through every row, joined at alternating ends: the longest parent chains there are

The baseline is the round trip these functions replace, for the regions alone: copy the map to the host, `scipy.ndimage.label` per
class, copy the labels back.  It is timed only where scipy imports and reported as absent otherwise; its partition is compared with
the device's first.  It is never the code under test: the tests compare with tests/regions_ref.py.

A repetition is one call between device events ending in a synchronise (the host round trip: wall clock around the whole of it);
median, min and max of --reps after --warmup calls.  Peak extra memory is `torch.cuda.max_memory_allocated` over one call less what
was allocated before it (results and workspaces included).

    python tools/regions_bench.py [--reps 7] [--warmup 2] [--size 4096]   ->  JSON lines
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def make_map(kind, size):
    rng = np.random.default_rng(0)
    if kind == "upsampled":
        return 10, np.repeat(np.repeat(rng.integers(0, 10, (size // 8, size // 8)), 8, 0), 8, 1).astype(np.int64)
    if kind == "percolation":
        return 2, (rng.random((size, size)) < 0.59).astype(np.int64)
    m = np.zeros((size, size), dtype=np.int64)
    m[::2] = 1
    for i, y in enumerate(range(1, size, 2)):
        m[y, size - 1 if i % 2 == 0 else 0] = 1
    return 2, m


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


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


def host_round_trip(labels, k):
    """The regions by way of the host: one `scipy.ndimage.label` per class (4-connectivity), ids made distinct across the classes."""
    m = labels.cpu().numpy()
    out = np.full(m.shape, -1, dtype=np.int64)
    base = 0
    for c in range(k):
        lab, n = ndimage.label(m == c)
        sel = lab > 0
        out[sel] = lab[sel] + (base - 1)
        base += n
    return torch.from_numpy(out).to(labels.device)


def _same_partition(dev, host):
    """Two labellings name the same regions: the pairs (device id, host id) are a bijection."""
    d, h = dev.reshape(-1), host.reshape(-1)
    if not torch.equal(d < 0, h < 0):
        return False
    keep = d >= 0
    pairs = torch.unique(torch.stack([d[keep], h[keep]]), dim=1)
    return pairs.shape[1] == torch.unique(d[keep]).numel() == torch.unique(h[keep]).numel()


def _stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}


def bench(kind, size, reps, warmup):
    k, m = make_map(kind, size)
    labels = torch.from_numpy(m).cuda()
    arms = {"label_regions": lambda: eae_amd.label_regions(labels, k),
            "majority_filter_r2": lambda: eae_amd.majority_filter(labels, k, radius=2),
            "sieve_16": lambda: eae_amd.sieve(labels, k, 16)}
    res = {"bench": "regions", "map": kind, "size": [size, size], "classes": k, "reps": reps}
    regions = arms["label_regions"]()
    res["regions"] = int(torch.unique(regions[regions >= 0]).numel())
    for name, fn in arms.items():
        peak = _peak_extra(fn)
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        res[name] = dict(_stats([_timed(fn) for _ in range(reps)]), peak_extra_bytes=peak)
    if ndimage is None:
        res["host_round_trip"] = None                                       # scipy is not installed: no baseline
    else:
        assert _same_partition(regions, host_round_trip(labels, k)), "the device and scipy.ndimage.label disagree"
        res["host_round_trip"] = _stats([_wall(lambda: host_round_trip(labels, k)) for _ in range(max(1, min(reps, 3)))])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--maps", default="upsampled,percolation,serpentine")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regions_bench needs a GPU: nothing is measured without one")
    for kind in a.maps.split(","):
        print(json.dumps(bench(kind, a.size, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
