#!/usr/bin/env python3
"""Nodata / mask path of scene classification:
  counts    eae_scene_invalid_counts (window_invalid_counts) time and HBM rate: 13-band uint16 10980 x 10980 (a Sentinel-2 tile, 3.1 GB)
            at S = 32, and RGB uint8 2112 x 2112 at S = 64, nodata = 0 plus a cloud mask.  Bytes: C * Hg * Wg * elem + Hg * Wg mask.
  classify  classify_scene(nodata=0) windows/s with 0 %, 50 % and 90 % of the windows invalid (a diagonal swath edge: every band 0
            beyond it) against the plain call on the same scene, 13-band uint16 2112 x 2112 at S = 32, B = 512.  The masked time
            includes the counts, the compaction and its one readback.
Timed with device events after a warm-up, median of --reps.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/scene_nodata_bench.py` run (scene_invalid_rows_kernel, scene_invalid_windows_kernel,
scene_select_kernel).

    python tools/scene_nodata_bench.py [--reps 7] [--warmup 2] [--only counts|classify]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402

B, P = 512, 64


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def counts(name, c, dtype, size, stride, reps, warmup):
    hi = 256 if dtype == torch.uint8 else 10000
    scene = torch.randint(1, hi, (c, size, size), dtype=torch.int32, device="cuda").to(dtype)
    scene[:, size // 2:, :size // 3] = 0
    mask = torch.zeros((size, size), dtype=torch.bool, device="cuda")
    mask[: size // 4, size // 2: size // 2 + size // 5] = True
    n_h, n_w = eae_amd.window_grid(size, size, P, stride)
    hg, wg = (n_h - 1) * stride + P, (n_w - 1) * stride + P
    nbytes = c * hg * wg * scene.element_size() + hg * wg

    def fn():
        eae_amd.window_invalid_counts(scene, P, stride, nodata=0, mask=mask)

    med, lo, hi_ = _time(fn, reps, warmup)
    tbs = nbytes / med / 1e12
    res = {"bench": "counts", "workload": name, "C": c, "dtype": str(dtype).replace("torch.", ""), "scene": [c, size, size],
           "stride": stride, "windows": n_h * n_w, "bytes": nbytes, "us": round(med * 1e6, 1), "min_us": round(lo * 1e6, 1),
           "max_us": round(hi_ * 1e6, 1), "TB_s": round(tbs, 3), "frac_8TBs": round(tbs / 8.0, 3), "frac_6p29TBs": round(tbs / 6.29, 3)}
    del scene, mask
    torch.cuda.empty_cache()
    return res


def _swath_offset(n_h, n_w, stride, frac):
    """d such that about `frac` of the windows reach beyond the diagonal x + y >= d (window (i, j) is invalid when its bottom-right
    pixel does: all bands are 0 there)."""
    i, j = np.mgrid[0:n_h, 0:n_w]
    far = (i * stride + P - 1) + (j * stride + P - 1)
    return int(np.quantile(far, 1.0 - frac)) if frac > 0 else 1 << 40


def classify(c, size, stride, reps, warmup):
    torch.manual_seed(0)
    model = eae_amd.SupervisedAutoencoder(64, 10, in_channels=c)
    model._eae_max_batch = B
    model = model.cuda().eval()
    mlp = eae_amd.MLP(64, 10).cuda().eval()
    base = torch.randint(1, 10000, (c, size, size), dtype=torch.int32, device="cuda").to(torch.uint16)
    n_h, n_w = eae_amd.window_grid(size, size, P, stride)
    yy = torch.arange(size, device="cuda")[:, None]
    xx = torch.arange(size, device="cuda")[None, :]
    out = []
    for frac in (0.0, 0.5, 0.9):
        d = _swath_offset(n_h, n_w, stride, frac)
        scene = base.clone()
        scene.view(torch.int16)[:, (yy + xx) >= d] = 0                 # (no masked fill for uint16; 0 has the same bits)
        nvalid = int(eae_amd.valid_windows(scene, P, stride, nodata=0).numel())

        def plain():
            eae_amd.classify_scene(scene, model, mlp, divisor=10000.0, stride=stride, batch=B)

        def masked():
            eae_amd.classify_scene(scene, model, mlp, divisor=10000.0, stride=stride, batch=B, nodata=0)

        res = {"bench": "classify", "C": c, "scene": [c, size, size], "stride": stride, "windows": n_h * n_w,
               "invalid_frac": round(1 - nvalid / (n_h * n_w), 3), "valid": nvalid}
        for tag, fn in (("plain", plain), ("nodata", masked)):
            med, lo, hi_ = _time(fn, reps, warmup)
            res[tag] = {"s": round(med, 5), "min_s": round(lo, 5), "max_s": round(hi_, 5), "windows_per_s": round(n_h * n_w / med, 1)}
        res["time_ratio"] = round(res["nodata"]["s"] / res["plain"]["s"], 3)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["counts", "classify"], default=None)
    a = ap.parse_args()
    if a.only in (None, "counts"):
        print(json.dumps(counts("s2_13band_u16", 13, torch.uint16, 10980, 32, a.reps, a.warmup)), flush=True)
        print(json.dumps(counts("rgb_u8", 3, torch.uint8, 2112, 64, a.reps, a.warmup)), flush=True)
    if a.only in (None, "classify"):
        for r in classify(13, 2112, 32, a.reps, a.warmup):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
