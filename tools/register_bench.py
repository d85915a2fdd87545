#!/usr/bin/env python3
"""The two co-registration kernels against torch routes on the same scenes.

- matching: `eae_match_tiles` on an 8192^2 uint16 pair, tile 64 / stride 256 (32 x 32 tiles), radius 8 and 16, against a torch
  route that converts the matched band to float, cuts out templates and windows, and forms the sums with `unfold` + batched products,
  --tile-chunk tiles at a time (the unfolded windows of 1024 tiles at radius 16 would take 18 GB).
- resampling: `eae_scene_resample` of 8192^2 x 4 uint16 for the three methods against float conversion + `affine_grid` +
  `grid_sample` (nearest / bilinear / bicubic, one band at a time above --band-chunk bands) + rounding back.  The floor is reading the
  source once and writing the destination once; TB/s counts those bytes.

The arms alternate after --warmup rounds; a repetition is --iters calls between device events; median, min and max per call over
--reps.  Peak extra memory is `torch.cuda.max_memory_allocated` over one call less what was allocated before it (for the kernels:
their outputs).  The outputs of the two routes are compared first.

    python tools/register_bench.py [--size 8192] [--reps 5] [--warmup 2] [--iters 3] [--tile-chunk 32] [--skip-torch]   ->  JSON lines
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANDS, TILE, STRIDE = 4, 64, 256


def scenes(size):
    """A textured uint16 scene and a copy shifted by (3, -2) pixels with a gain, built band by band."""
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.empty((BANDS, size, size), dtype=torch.uint16, device="cuda")
    b = torch.empty_like(a)
    for i in range(BANDS):
        x = torch.randint(0, 3000, (size // 4, size // 4), device="cuda", generator=g, dtype=torch.int32)
        x = x.repeat_interleave(4, 0).repeat_interleave(4, 1) + torch.randint(0, 1000, (size, size), device="cuda", generator=g, dtype=torch.int32)
        a[i] = x.to(torch.uint16)
        b[i] = (x.roll((-2, 3), (0, 1)) * 9 // 10 + 50).to(torch.uint16)
    return a, b


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def _measure(arms, reps, warmup, iters):
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, fn in arms.items():
            ms = _timed(fn, iters)
            if r >= warmup:
                times[k].append(ms)
    return {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}


def torch_match(a, b, oa, radius, chunk):
    """float64 [n, (2R + 1)^2, 6] of an all-valid pair: unfold + batched products over the feature band."""
    nd, t = 2 * radius + 1, TILE
    fa, fb = a[0].to(torch.float32), b[0].to(torch.float32)
    fb = torch.nn.functional.pad(fb, (radius, radius, radius, radius))
    out = []
    for lo in range(0, len(oa), chunk):
        tm = torch.stack([fa[y:y + t, x:x + t] for y, x in oa[lo:lo + chunk]]).reshape(-1, 1, t * t)
        win = torch.stack([fb[y:y + t + 2 * radius, x:x + t + 2 * radius] for y, x in oa[lo:lo + chunk]])
        u = torch.nn.functional.unfold(win[:, None], t)                                  # [n, T^2, ND^2]
        sab = (tm @ u)[:, 0]
        sb, sbb = u.sum(1), (u * u).sum(1)
        sa, saa = tm.sum(2).expand(-1, nd * nd), (tm * tm).sum(2).expand(-1, nd * nd)
        out.append(torch.stack([torch.full_like(sab, t * t), sa, sb, saa, sbb, sab], 2))
    return torch.cat(out)


def bench_match(a, b, radius, args):
    from eae_amd import _lib
    from eae_amd.engine import _ptr, _stream
    lib = _lib.load()
    c, h, w = a.shape
    ys = range(0, h - TILE + 1, STRIDE)
    oa = [(y, x) for y in ys for x in range(0, w - TILE + 1, STRIDE)]
    n, nd = len(oa), 2 * radius + 1
    org = torch.tensor(oa, dtype=torch.int32, device="cuda")
    div = torch.full((c,), 4095.0, device="cuda")
    sums = torch.empty((n, nd * nd, 6), dtype=torch.int64, device="cuda")

    def kernel():
        _lib.check(lib.eae_match_tiles(_stream(), _ptr(a), 1, c, h, w, 0, _ptr(div), 0, 0.0, 0, None, _ptr(b), 1, c, h, w, 0, _ptr(div),
                                       0, 0.0, 0, None, TILE, radius, n, _ptr(org), _ptr(org), _ptr(sums)))
        return sums

    arms = {"kernel": kernel}
    out = {"what": "match_tiles", "scene": [c, h, w], "tile": TILE, "stride": STRIDE, "radius": radius, "tiles": n,
           "kernel_extra_bytes": sums.numel() * 8}
    kernel()
    cnt = sums[:, :, 0]
    inside = cnt == TILE * TILE                                                          # the torch route pads B with zeros instead
    if not args.skip_torch:
        arms["torch"] = lambda: torch_match(a, b, oa, radius, args.tile_chunk)
        ref = arms["torch"]()
        k = sums.double()
        # the raw values (not the features) enter the torch route: compare the correlation, which is invariant to the scaling
        def score(s):
            num = s[..., 0] * s[..., 5] - s[..., 1] * s[..., 2]
            return num / torch.sqrt((s[..., 0] * s[..., 3] - s[..., 1] ** 2) * (s[..., 0] * s[..., 4] - s[..., 2] ** 2))
        out["score_abs_diff"] = float((score(k) - score(ref.double()))[inside].abs().max())
        out["torch_extra_bytes"] = _peak(arms["torch"])
        del ref
    out.update(_measure(arms, args.reps, args.warmup, args.iters))
    print(json.dumps(out), flush=True)


def torch_resample(src, theta, mode, band_chunk):
    c, h, w = src.shape
    grid = torch.nn.functional.affine_grid(theta[None], (1, 1, h, w), align_corners=True)
    out = torch.empty_like(src)
    for lo in range(0, c, band_chunk):
        f = src[None, lo:lo + band_chunk].to(torch.float32)
        r = torch.nn.functional.grid_sample(f, grid, mode=mode, padding_mode="zeros", align_corners=True)
        out[lo:lo + band_chunk] = r[0].round().clamp(0, 65535).to(torch.uint16)
    return out


def bench_resample(a, args):
    from eae_amd import _lib
    from eae_amd.engine import _ptr, _stream
    lib = _lib.load()
    c, h, w = a.shape
    t = math.radians(0.3)
    cs, sn = 1.002 * math.cos(t), 1.002 * math.sin(t)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    m = np.array([[cs, -sn, cx - cs * cx + sn * cy + 3.4], [sn, cs, cy - sn * cx - cs * cy - 2.7]])
    norm = np.array([[2.0 / (w - 1), 0.0, -1.0], [0.0, 2.0 / (h - 1), -1.0], [0.0, 0.0, 1.0]])
    theta = torch.tensor((norm @ np.vstack([m, [0.0, 0.0, 1.0]]) @ np.linalg.inv(norm))[:2], dtype=torch.float32, device="cuda")
    dst = torch.empty_like(a)
    valid = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    floor_bytes = 2 * a.numel() * a.element_size()
    for method, (mid, mode) in {"nearest": (0, "nearest"), "bilinear": (1, "bilinear"), "cubic": (2, "bicubic")}.items():
        def kernel():
            _lib.check(lib.eae_scene_resample(_stream(), _ptr(a), 1, c, h, w, 0, 0.0, 0, None, m.ctypes.data, mid, 0.0, _ptr(dst), h, w,
                                              _ptr(valid)))
            return dst

        arms = {"kernel": kernel}
        out = {"what": "scene_resample", "scene": [c, h, w], "method": method, "floor_bytes": floor_bytes,
               "kernel_extra_bytes": dst.numel() * 2 + valid.numel()}
        kernel()
        if not args.skip_torch:
            arms["torch"] = lambda: torch_resample(a, theta, mode, args.band_chunk)
            ref = arms["torch"]()
            inner = valid.bool()
            diff = (dst.to(torch.int32) - ref.to(torch.int32)).abs()[:, inner]
            # torch's bicubic uses a = -0.75, and its fp32 coordinates move a tap by up to 2^-11 px at 8192: not the same numbers
            out["max_abs_diff_vs_torch"] = int(diff.max())
            out["mean_abs_diff_vs_torch"] = float(diff.float().mean())
            out["torch_extra_bytes"] = _peak(arms["torch"])
            del ref, diff
        res = _measure(arms, args.reps, args.warmup, args.iters)
        res["kernel"]["TBps"] = round(floor_bytes / res["kernel"]["ms"] / 1e9, 3)
        out.update(res)
        out["valid_share"] = float(valid.float().mean())
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--tile-chunk", type=int, default=32)
    ap.add_argument("--band-chunk", type=int, default=1)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--only", choices=("match", "resample"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("register_bench needs a HIP device")
    a, b = scenes(args.size)
    if args.only != "resample":
        for radius in (8, 16):
            bench_match(a, b, radius, args)
            torch.cuda.empty_cache()
    if args.only != "match":
        del b
        bench_resample(a, args)


if __name__ == "__main__":
    main()
