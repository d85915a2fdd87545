#!/usr/bin/env python3
"""Scene reconstruction throughput (windows/s): scene_reconstruction_error and reconstruct_scene(residual=True) (deconv4 reads its
MSE target from the scene, one C call) against the staged composition of older public pieces (scene_windows -> model(x) -> a torch
MSE per window, batch by batch), with B = 512 windows per pass, on
  rgb8   RGB uint8 scene                      ms16   13-band uint16 scene (Sentinel-2-like, divisor 10000)
each at S = P (non-overlapping windows) and S = P/2, scenes sized for at least 16 K windows.  Timed with device events after a
warm-up (medians).  `edge_bytes` are the algorithmic bytes per window of the two edge layers and what surrounds them (everything
between conv1's output and deconv4's input is the same in both routes): with e the scene's element size,
  staged          C P^2 (e + 20)    gather read + fp32 batch write, conv1 read, x_hat write, MSE reading both batches
  fused error     2 C P^2 e         conv1 and deconv4's target read the scene
  fused stitched  2 C P^2 e + 4 S^2 (C + 1)    ... plus the owned pixels of x_hat and the residual

    python tools/scene_recon_bench.py [--reps 5] [--warmup 2] [--only rgb8|ms16]   ->  JSON lines
"""
import argparse
import json
import os
import sys

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


def run(name, c, dtype, stride, divisor, size, reps, warmup):
    torch.manual_seed(0)
    model = eae_amd.SupervisedAutoencoder(64, 10, in_channels=c)
    model._eae_max_batch = B
    model = model.cuda().eval()
    hi = 256 if dtype == torch.uint8 else 10000
    scene = torch.randint(0, hi, (c, size, size), dtype=torch.int32, device="cuda").to(dtype)
    n_h, n_w = eae_amd.window_grid(size, size, P, stride)
    n = n_h * n_w
    e = scene.element_size()

    def fused_error():
        return eae_amd.scene_reconstruction_error(scene, model, divisor=divisor, stride=stride, batch=B)

    def fused_stitched():
        return eae_amd.reconstruct_scene(scene, model, divisor=divisor, stride=stride, batch=B, residual=True)

    def staged():
        outs = []
        with torch.no_grad():
            for b0 in range(0, n, B):
                x = eae_amd.scene_windows(scene, divisor, P, stride, first=b0, count=min(B, n - b0))
                outs.append(((model(x)[0] - x) ** 2).mean(dim=(1, 2, 3)))
        return torch.cat(outs).reshape(n_h, n_w)

    # the routes agree before they are timed
    rel = ((fused_error() - staged()).abs() / staged()).max().item()
    res = {"workload": name, "C": c, "dtype": str(dtype).replace("torch.", ""), "stride": stride, "scene": [c, size, size],
           "windows": n, "batch": B, "max_rel_diff": rel,
           "edge_bytes": {"staged": c * P * P * (e + 20), "fused_error": 2 * c * P * P * e,
                          "fused_stitched": 2 * c * P * P * e + 4 * stride * stride * (c + 1)}}
    for tag, fn in (("fused_error", fused_error), ("fused_stitched", fused_stitched), ("staged", staged)):
        med, lo, hi_ = _time(fn, reps, warmup)
        res[tag] = {"s": round(med, 5), "min_s": round(lo, 5), "max_s": round(hi_, 5), "windows_per_s": round(n / med, 1)}
    res["speedup_error"] = round(res["staged"]["s"] / res["fused_error"]["s"], 3)
    res["speedup_stitched"] = round(res["staged"]["s"] / res["fused_stitched"]["s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["rgb8", "ms16"], default=None)
    a = ap.parse_args()
    # 128 x 128 = 16 384 windows at S = P, 129 x 129 = 16 641 at S = P/2
    work = [("rgb8", 3, torch.uint8, 255.0), ("ms16", 13, torch.uint16, 10000.0)]
    for name, c, dtype, div in work:
        if a.only and a.only != name:
            continue
        for stride, size in ((P, 128 * P), (P // 2, 128 * (P // 2) + P)):
            print(json.dumps(run(name, c, dtype, stride, div, size, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
