#!/usr/bin/env python3
"""Zonal statistics of a cell map inside the zones of a zone raster: `zonal_stats` with probabilities (one kernel reading the raster
once; integer tables) against the torch route (upsample the cell map and the K probability planes with `repeat_interleave`, form
zones * (K + 1) + label as H x W int64, one `bincount`, K float64 `index_add_` calls).  8192 x 8192 int32 zones, K = 10, cells of 16:

    parcels   jittered blocks of about 64 x 64 pixels, roughly 16 K zones (field parcels that do not follow the cell grid);
    regions   `label_regions` of a noisy map, compacted: about 10^6 small zones (the adversarial case: little to merge).

The vote tables are asserted equal first, and the probability sums equal to the float64 route's within its rounding.  Then the arms
alternate inside one process after --warmup rounds; a repetition is one call between device events, ending in a synchronise; median,
min and max of --reps.  TB/s counts the zone raster's bytes, the bytes the algorithm has to read.  Each arm's peak extra allocation is
`torch.cuda.max_memory_allocated` over one call less what was allocated before it.  `paint_zones` is timed the same way against
`values[zones]` (TB/s: the ids read plus the int64 raster written).  The kernel alone comes from a separate `rocprofv3
--kernel-trace --stats -- python tools/zonal_bench.py` run (zonal_accumulate_kernel, zonal_paint_kernel).

--no-probs times the votes alone (no probabilities on either route: `zonal_stats` without `probs`, the torch route without its
`index_add_`s), which separates the cost of the K probability adds of a flush from the rest.

    python tools/zonal_bench.py [--reps 7] [--warmup 2] [--size 8192] [--case parcels|regions|both] [--no-probs]   ->  JSON lines
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


def torch_route(zones, z, labels, probs=None):
    h, w = zones.shape
    up = labels.repeat_interleave(CELL, 0).repeat_interleave(CELL, 1)[:h, :w]
    c = torch.where((up >= 0) & (up < K), up, K)
    zl = zones.to(torch.int64)
    ok = (zl >= 0) & (zl < z)
    votes = torch.bincount((zl * (K + 1) + c)[ok], minlength=z * (K + 1)).reshape(z, K + 1)
    if probs is None:
        return votes, None
    sel = ok & (c < K)
    zsel = zl[sel]
    sums = torch.zeros((K, z), dtype=torch.float64, device=zones.device)
    for j in range(K):
        pj = probs[j].repeat_interleave(CELL, 0).repeat_interleave(CELL, 1)[:h, :w]
        sums[j].index_add_(0, zsel, pj[sel].to(torch.float64))
    return votes, sums.t()


def torch_paint(zones, values):
    zl = zones.to(torch.int64)
    ok = (zl >= 0) & (zl < values.numel())
    return torch.where(ok, values[torch.where(ok, zl, 0)], -1)


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


def parcel_zones(size, g):
    """Blocks of 64 x 64 whose column boundaries shift per band of 64 rows and whose row boundaries shift per band of 64 columns."""
    nb = size // 64 + 1
    dx = torch.randint(0, 64, (nb,), generator=g)
    dy = torch.randint(0, 64, (nb,), generator=g)
    y, x = torch.arange(size)[:, None], torch.arange(size)[None, :]
    zones = ((y + dy[x // 64]) // 64) * (nb + 1) + (x + dx[y // 64]) // 64
    return zones.to(torch.int32).cuda(), (nb + 1) * (nb + 1)


def region_zones(size, g):
    """`label_regions` of a map of 8 x 8 blocks of one class with 0.5 % single-pixel noise, compacted."""
    coarse = torch.randint(0, K, (size // 8, size // 8), generator=g)
    m = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1)
    noise = torch.rand((size, size), generator=g) < 0.005
    m = torch.where(noise, torch.randint(0, K, (size, size), generator=g), m).cuda()
    zones, ids = eae_amd.compact_zones(eae_amd.label_regions(m, K))
    return zones, int(ids.numel())


def _stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def bench(case, size, reps, warmup, with_probs=True):
    g = torch.Generator().manual_seed(size)
    zones, z = (parcel_zones if case == "parcels" else region_zones)(size, g)
    c = -(-size // CELL)
    labels = torch.randint(-1, K, (c, c), generator=g).cuda()
    probs = torch.softmax(torch.randn((K, c, c), generator=g) * 2, 0).cuda() if with_probs else None
    arms = {"zonal_stats": lambda: eae_amd.zonal_stats(zones, z, labels, K, probs=probs, cell=CELL),
            "torch_index_add": lambda: torch_route(zones, z, labels, probs)}
    a, b = (fn() for fn in arms.values())
    assert torch.equal(a.votes, b[0]), "the vote tables disagree"
    if with_probs:
        got = a.prob_sums.to(torch.float64) / 2.0 ** 32
        assert bool(((got - b[1]).abs() <= 1e-6 * b[1].abs() + 1e-6).all()), "the probability sums disagree"
    assert int(a.votes.sum()) == size * size
    again = arms["zonal_stats"]()
    assert torch.equal(again.votes, a.votes), "two runs differ"
    assert not with_probs or torch.equal(again.prob_sums, a.prob_sums), "two runs differ"
    values = eae_amd.zone_labels(a, "probs" if with_probs else "votes")[0]
    del a, b, again
    paint = {"paint_zones": lambda: eae_amd.paint_zones(zones, values), "torch_gather": lambda: torch_paint(zones, values)}
    pa, pb = (fn() for fn in paint.values())
    assert torch.equal(pa, pb), "the painted rasters disagree"
    del pa, pb
    arms.update(paint)
    peak = {k: _peak_extra(fn) for k, fn in arms.items()}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():                           # alternating
            ts[k].append(_timed(fn))
    nbytes = {k: size * size * (4 if k in ("zonal_stats", "torch_index_add") else 12) for k in arms}
    res = {"bench": "zonal_stats", "case": case, "zones": [size, size], "dtype": "int32", "num_zones": z, "classes": K, "cell": CELL,
           "probs": bool(with_probs), "reps": reps}
    for k, v in ts.items():
        res[k] = dict(_stats(v), bytes=nbytes[k], peak_extra_bytes=peak[k])
        res[k]["tb_per_s"] = round(nbytes[k] / (res[k]["ms"] * 1e-3) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--case", choices=("parcels", "regions", "both"), default="both")
    ap.add_argument("--no-probs", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zonal_bench needs a GPU: nothing is measured without one")
    for case in (("parcels", "regions") if a.case == "both" else (a.case,)):
        print(json.dumps(bench(case, a.size, a.reps, a.warmup, not a.no_probs)), flush=True)


if __name__ == "__main__":
    main()
