#!/usr/bin/env python3
"""One IR-MAD iteration on the device against a chunked torch route on the same scenes.

- kernels: `eae_change_moments` (weights given) and `eae_change_variates` (only prob written), the two passes of an iteration, each
  timed alone and together; the workspace and the outputs are allocated once, as `mad_fit` would reuse them.
- torch: for every chunk of --chunk pixels the float conversion of both scenes into a [2C, n] matrix, the weighted ``d @ d.T``, and a
  matmul for the variates with ``torch.special.gammaincc`` for prob.

Shapes (C, H, W, dtype): 8192^2 x 4 uint16, 8192^2 x 3 uint8, 4096^2 x 16 uint16 (--shape picks one).  The arms alternate after
--warmup rounds; a repetition is --iters calls between device events; median, min and max per call over --reps.  TB/s counts the two
scenes' bytes once per pass.  Peak extra memory is `torch.cuda.max_memory_allocated` over one call less what was allocated before it.
The covariance of the two routes is compared first (largest difference relative to the largest element).

    python tools/change_bench.py [--shape 0] [--reps 5] [--warmup 2] [--iters 3] [--chunk 4194304]   ->  JSON lines
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 8192, 8192, torch.uint16), (3, 8192, 8192, torch.uint8), (16, 4096, 4096, torch.uint16)]


def scenes(c, h, w, dtype):
    """Two correlated scenes built band by band (no float copy of a whole scene), a weight raster, a pivot and a model."""
    g = torch.Generator(device="cuda").manual_seed(0)
    top = 4096 if dtype == torch.uint16 else 256
    a = torch.empty((c, h, w), dtype=dtype, device="cuda")
    b = torch.empty((c, h, w), dtype=dtype, device="cuda")
    for i in range(c):
        x = torch.randint(0, top, (h, w), device="cuda", generator=g, dtype=torch.int32)
        a[i] = x.to(dtype)
        b[i] = ((x * 3 + torch.randint(0, top, (h, w), device="cuda", generator=g, dtype=torch.int32)) // 4).to(dtype)
    weights = torch.rand((h, w), device="cuda", generator=g)
    pivot = torch.full((2 * c,), top / 2.0, device="cuda")
    t = torch.randn((2 * c, c), device="cuda", generator=g) / (top * (2 * c) ** 0.5)
    return a, b, weights, pivot, t.contiguous()


def torch_iteration(a, b, div, weights, pivot, t, chunk):
    c, h, w = a.shape
    af, bf, wf = a.reshape(c, -1), b.reshape(c, -1), weights.reshape(-1)
    s2 = torch.zeros((2 * c, 2 * c), device=a.device)
    s1 = torch.zeros(2 * c, device=a.device)
    n = torch.zeros((), device=a.device)
    prob = torch.empty(h * w, device=a.device)
    for lo in range(0, h * w, chunk):
        v = torch.cat([af[:, lo:lo + chunk].to(torch.float32) / div, bf[:, lo:lo + chunk].to(torch.float32) / div])
        d = v - pivot[:, None]
        dw = d * wf[lo:lo + chunk]
        s2 += dw @ d.T
        s1 += dw.sum(1)
        n += wf[lo:lo + chunk].sum()
        z = (t.T @ d).square().sum(0)
        prob[lo:lo + chunk] = torch.special.gammaincc(torch.full_like(z, c / 2.0), z / 2.0)
    return n, s1, s2, prob.reshape(h, w)


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
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run(shape, reps, warmup, iters, chunk):
    from eae_amd import _lib
    from eae_amd.engine import _ptr, _stream
    from eae_amd.scene import _DTYPES
    c, h, w, dtype = shape
    a, b, weights, pivot, t = scenes(c, h, w, dtype)
    lib = _lib.load()
    div = torch.ones(c, device="cuda")
    nbytes = lib.eae_change_moments_workspace_bytes(c, h, w)
    base = torch.cuda.memory_allocated()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mom = torch.empty(1 + 2 * c + 4 * c * c, dtype=torch.float64, device="cuda")
    count = torch.empty(1, dtype=torch.int64, device="cuda")
    prob = torch.empty((h, w), device="cuda")
    extra = torch.cuda.memory_allocated() - base
    head = (_ptr(a), _ptr(b), _DTYPES[dtype], _DTYPES[dtype], c, h, w, _ptr(div), _ptr(div), 0, 0.0, 0, 0, 0.0, 0, None)

    def moments():
        _lib.check(lib.eae_change_moments(_stream(), *head, _ptr(weights), _ptr(pivot), _ptr(mom), _ptr(count), _ptr(ws), nbytes))

    def variates():
        _lib.check(lib.eae_change_variates(_stream(), *head, _ptr(pivot), _ptr(t), c, None, _ptr(prob), None))

    def both():
        moments()
        variates()

    def torch_arm():
        return torch_iteration(a, b, div[:, None], weights, pivot, t, chunk)

    both()
    n, s1, s2, tprob = torch_arm()
    m = mom.cpu()
    s2k = m[1 + 2 * c:].reshape(2 * c, 2 * c)
    cov_diff = float((s2k - s2.cpu().double()).abs().max() / s2k.abs().max())
    prob_diff = float((prob - tprob).abs().max())
    del n, s1, s2, tprob
    arms = {"moments": moments, "variates": variates, "iteration": both, "torch": torch_arm}
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, fn in arms.items():
            ms = _timed(fn, iters)
            if r >= warmup:
                times[k].append(ms)
    scene_bytes = 2 * c * h * w * a.element_size()
    out = {"shape": [c, h, w], "dtype": str(dtype).replace("torch.", ""), "scene_bytes_per_pass": scene_bytes,
           "workspace_bytes": nbytes, "kernel_extra_bytes": extra, "torch_extra_bytes": _peak(torch_arm),
           "cov_rel_diff": cov_diff, "prob_abs_diff": prob_diff, "count": int(count.cpu()[0])}
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"ms": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        if k in ("moments", "variates"):
            out[k]["TBps"] = round(scene_bytes / med / 1e9, 3)
    out["iteration"]["TBps"] = round(2 * scene_bytes / out["iteration"]["ms"] / 1e9, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=None, help="index into the shape list (default: all, one after the other)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("change_bench needs a HIP device")
    for i in range(len(SHAPES)) if args.shape is None else [args.shape]:
        run(SHAPES[i], args.reps, args.warmup, args.iters, args.chunk)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
