#!/usr/bin/env python3
"""Scene classification throughput (windows/s): classify_scene (conv1 reads the scene, one C call) against the staged composition
(scene_windows -> eval Encoder -> MLP eval, batch by batch), on two workloads with B = 512 windows per encoder pass:
  rgb8   RGB uint8 scene at S = 64 (non-overlapping windows)
  ms16   13-band uint16 scene at S = 32 (Sentinel-2-like, divisor 10000)
Timed with device events after a warm-up; the staged path also reports its fp32 staging bytes.  Per-kernel times of the fused conv1
come from a separate `rocprofv3 --kernel-trace --stats -- python tools/scene_bench.py` run (edge_conv_scene_kernel).

--border MODE adds a border leg to each workload: the scene cropped by CROP pixels per axis, so that its virtual padded grid is the
grid of the uncropped scene, classified with border=MODE (the kernels resolve the padding) against the path without the feature:
a padded device copy made with torch indexing, then the borderless classify_scene, the copy inside the timed region.  The two are
timed alternately and their outputs compared bitwise; "pad_copy_bytes" is the extra device memory of the padded copy.

    python tools/scene_bench.py [--reps 5] [--warmup 2] [--size 2112] [--border reflect]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd.mlp_engine import mlp_engine_for  # noqa: E402

B, P = 512, 64
CROP = 20          # border leg: pixels cut off each axis (centre pads 10 / 10)


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


def _time_alternating(fns, reps, warmup):
    """Median / min / max seconds of each function, the functions taking turns inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) / 1e3)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def border_leg(scene, model, mlp, divisor, stride, mode, reps, warmup):
    size = scene.shape[1]
    real = scene[:, :size - CROP, :size - CROP].contiguous()
    n_h, n_w, (pt, pb, pl, pr) = eae_amd.border_grid(size - CROP, size - CROP, P, stride)
    src = [torch.tensor([eae_amd.border_source(v, lead, size - CROP, mode) or 0 for v in range(size - CROP + lead + trail)],
                        device="cuda") for lead, trail in ((pt, pb), (pl, pr))]
    inside = [torch.tensor([eae_amd.border_source(v, lead, size - CROP, mode) is not None
                            for v in range(size - CROP + lead + trail)], device="cuda") for lead, trail in ((pt, pb), (pl, pr))]
    raw = real.view(torch.int16) if real.dtype == torch.uint16 else real       # torch indexes no uint16 tensors

    def pad_copy():
        out = raw[:, src[0][:, None], src[1][None, :]]
        if mode == "constant":
            out = out * (inside[0][:, None] & inside[1][None, :]).to(out.dtype)      # fill = 0
        return out.view(real.dtype)

    def bordered():
        return eae_amd.classify_scene(real, model, mlp, divisor=divisor, stride=stride, batch=B, border=mode)

    def padded():
        return eae_amd.classify_scene(pad_copy(), model, mlp, divisor=divisor, stride=stride, batch=B)

    same = all(torch.equal(x, y) for x, y in zip(bordered(), padded()))
    res = {"mode": mode, "scene": list(real.shape), "pads": [pt, pb, pl, pr], "windows": n_h * n_w, "bitwise_equal": same,
           "pad_copy_bytes": (size - CROP + pt + pb) * (size - CROP + pl + pr) * real.shape[0] * real.element_size()}
    for tag, (med, lo, hi) in zip(("border", "pad_copy_then_borderless"), _time_alternating((bordered, padded), reps, warmup)):
        res[tag] = {"s": round(med, 5), "min_s": round(lo, 5), "max_s": round(hi, 5), "windows_per_s": round(n_h * n_w / med, 1)}
    res["speedup"] = round(res["pad_copy_then_borderless"]["s"] / res["border"]["s"], 3)
    return res


def run(name, c, dtype, stride, divisor, size, reps, warmup, border=None):
    torch.manual_seed(0)
    model = eae_amd.SupervisedAutoencoder(64, 10, in_channels=c)
    model._eae_max_batch = B
    model = model.cuda().eval()
    mlp = eae_amd.MLP(64, 10).cuda().eval()
    hi = 256 if dtype == torch.uint8 else 10000
    scene = torch.randint(0, hi, (c, size, size), dtype=torch.int32, device="cuda").to(dtype)
    n_h, n_w = eae_amd.window_grid(size, size, P, stride)
    n = n_h * n_w
    meng = mlp_engine_for(mlp, max_batch=B)

    def fused():
        eae_amd.classify_scene(scene, model, mlp, divisor=divisor, stride=stride, batch=B)

    def staged():
        outs = []
        with torch.no_grad():
            for b0 in range(0, n, B):
                nb = min(B, n - b0)
                z = model.enc(eae_amd.scene_windows(scene, divisor, P, stride, first=b0, count=nb))
                outs.append(meng.forward(z))
        logits = torch.cat(outs)
        return torch.softmax(logits, 1), logits.argmax(1)

    res = {"workload": name, "C": c, "dtype": str(dtype).replace("torch.", ""), "stride": stride, "scene": [c, size, size],
           "windows": n, "batch": B, "staging_bytes": n * c * P * P * 4}
    for tag, fn in (("fused", fused), ("staged", staged)):
        med, lo, hi_ = _time(fn, reps, warmup)
        res[tag] = {"s": round(med, 5), "min_s": round(lo, 5), "max_s": round(hi_, 5), "windows_per_s": round(n / med, 1)}
    res["speedup"] = round(res["staged"]["s"] / res["fused"]["s"], 3)
    if border:
        res["border"] = border_leg(scene, model, mlp, divisor, stride, border, reps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=2112, help="scene height = width in pixels")
    ap.add_argument("--only", choices=["rgb8", "ms16"], default=None)
    ap.add_argument("--border", choices=["constant", "edge", "reflect"], default=None, help="add the border leg (module docstring)")
    a = ap.parse_args()
    work = [("rgb8", 3, torch.uint8, 64, 255.0), ("ms16", 13, torch.uint16, 32, 10000.0)]
    for name, c, dtype, stride, div in work:
        if a.only and a.only != name:
            continue
        print(json.dumps(run(name, c, dtype, stride, div, a.size, a.reps, a.warmup, a.border)), flush=True)


if __name__ == "__main__":
    main()
