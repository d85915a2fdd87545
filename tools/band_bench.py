#!/usr/bin/env python3
"""Joint train step (forward, 35*MSE + CE, backward, Adam) at B=512, 64x64, for C image bands (in_channels), timed with device
events after a warm-up; and the five edge launch sites stand-alone (through the C-band op entry points, back to back) with
their HBM fraction from the SURVEY 8d byte model at C bands (x = C*H*W fp32 elements per image, deconv4's bf16 gradient
g = CP*H*W, the 32-channel maps at H/2 in bf16; the train step writes no x_hat).  In-step per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/band_bench.py --bands 3 13 --no-sites` run (kernel names carry CP as their
last template argument); `--prof-db DIR/run_results.db` prints them with the same model.

    python tools/band_bench.py [--bands 3 4 8 13 16] [--sites 3 13] [--steps 50] [--warmup 10]   ->  JSON lines
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd.engine import engine_for  # noqa: E402

B, H = 512, 64
HBM_GBS = 8000.0


def edge_bytes(c, h=H):
    """Bytes per image of the five edge launch sites (SURVEY 8d model at C bands)."""
    cp = 4 if c == 3 else 8 if c <= 8 else 16
    x, g = 4 * c * h * h, 2 * cp * h * h          # fp32 image, bf16 NHWC-CP gradient
    y1 = 2 * 32 * (h // 2) ** 2                    # bf16 32-channel map at h/2
    return {"conv1_fwd": x + y1,                   # read x, write y1
            "deconv4_loss": y1 + x + g,            # read a3 and the target, write g (no x_hat in the train step)
            "deconv4_bwd_data": g + 2 * y1,        # read g and the previous map (mask), write the gradient map
            "conv1_wgrad": x + 2 * y1,             # read x, the gradient map and y1 (BatchNorm backward on load)
            "deconv4_wgrad": g + y1}               # read g and a3


def run(c, steps, warmup):
    torch.manual_seed(0)
    m = eae_amd.SupervisedAutoencoder(64, in_channels=c).cuda()
    eng = engine_for(m, max_batch=B)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((B, c, H, H), device="cuda", generator=g)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    for _ in range(warmup):
        eng.train_step(x, y, 35.0, 5e-3)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.train_step(x, y, 35.0, 5e-3)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    mb = {k: v * B / 1e6 for k, v in edge_bytes(c).items()}
    return {"bands": c, "batch": B, "ms_per_step": round(ms, 4), "images_per_s": round(B / ms * 1e3),
            "edge_MB_per_step": {k: round(v, 1) for k, v in mb.items()},
            "edge_us_at_hbm_peak": {k: round(v / HBM_GBS * 1e3, 1) for k, v in mb.items()},
            "final_loss": float(eng.loss_last[0])}


def sites(c, reps=20):
    """Stand-alone time (us) of the five edge launch sites at C bands, B=512, and their HBM fraction."""
    from eae_amd import _lib as L
    lib = L.load()
    dev = "cuda"
    cp = 4 if c == 3 else 8 if c <= 8 else 16
    kp = (9 * cp + 31) // 32 * 32
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    h2 = H // 2
    x = torch.rand((B, c, H, H), device=dev)
    g = (torch.randn((B, H, H, cp), device=dev) * 1e-3).to(torch.bfloat16)
    y = torch.randn((B, h2, h2, 32), device=dev).to(torch.bfloat16)
    y2 = torch.randn((B, h2, h2, 32), device=dev).to(torch.bfloat16)
    out = torch.empty((B, h2, h2, 32), device=dev, dtype=torch.bfloat16)
    w = torch.randn((32, c, 3, 3), device=dev) * 0.1
    wpack = torch.zeros(32 * kp, dtype=torch.bfloat16, device=dev)
    wjoint = torch.zeros(4 * cp * 128, dtype=torch.bfloat16, device=dev)
    L.check(lib.eae_op_pack_edge(st, p(w), c, p(wpack), p(wjoint)))
    bias = torch.zeros(32, device=dev)
    nt = B * (h2 // 4) * (h2 // 32)
    part = torch.zeros((2, 32, nt), device=dev)
    coef4 = torch.cat([torch.ones(32, device=dev), torch.zeros(32, device=dev), torch.zeros(32, device=dev), torch.ones(32, device=dev)])
    coef3 = torch.cat([torch.ones(32, device=dev), torch.full((32,), 1e-3, device=dev), torch.zeros(32, device=dev)])
    lp = torch.zeros(nt * ((c + 4) // 4 * 4), device=dev)
    scratch = torch.zeros(2048 * 288 * c, device=dev)
    dw = torch.zeros(32 * 9 * c, device=dev)
    side_bnbwd = L.EaeSrc(y.data_ptr(), y2.data_ptr(), coef3.data_ptr(), 2)
    side_bnrelu = L.EaeSrc(y.data_ptr(), None, coef4.data_ptr(), 1)
    a3 = L.EaeSrc(y.data_ptr(), None, coef4.data_ptr(), 1)
    calls = {
        "conv1_fwd": lambda: lib.eae_op_edge_conv_c(st, 0, p(x), c, B, H, H, p(wpack), p(bias), p(out), p(part), 0, None, None),
        "deconv4_loss": lambda: lib.eae_op_deconv4_loss_c(st, a3, c, B, h2, h2, p(wjoint), p(bias), p(x), C.c_float(1e-6), None, p(g), p(lp)),
        "deconv4_bwd_data": lambda: lib.eae_op_edge_conv_c(st, 1, p(g), c, B, H, H, p(wpack), None, p(out), p(part), 1, p(y2), p(coef4)),
        "conv1_wgrad": lambda: lib.eae_op_edge_wgrad_c(st, 0, p(x), c, B, H, H, side_bnbwd, p(scratch), scratch.numel(), p(dw)),
        "deconv4_wgrad": lambda: lib.eae_op_edge_wgrad_c(st, 1, p(g), c, B, H, H, side_bnrelu, p(scratch), scratch.numel(), p(dw)),
    }
    mb = {k: v * B / 1e6 for k, v in edge_bytes(c).items()}
    res = {}
    for k, fn in calls.items():
        for _ in range(3):
            L.check(fn())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        res[k] = {"us": round(us, 1), "MB": round(mb[k], 1), "hbm_frac": round(mb[k] / (us * HBM_GBS / 1e3), 3)}
    return {"bands": c, "standalone": res}


def prof_db(path, bands):
    """In-step per-kernel averages of a rocprofv3 kernel trace of this tool, with the byte model's HBM fraction."""
    import sqlite3
    import statistics
    fam = {("edge_conv_kernel", "0, 0"): "conv1_fwd", ("edge_conv_kernel", "1, 1"): "deconv4_bwd_data",
           ("edge_wgrad_kernel", "0, 2"): "conv1_wgrad", ("edge_wgrad_kernel", "1, 1"): "deconv4_wgrad", ("deconv4_loss_kernel", "1"): "deconv4_loss"}
    d = {}
    for name, dur in sqlite3.connect(path).execute("select name, duration from kernels"):
        m = re.match(r"(?:void )?(\w+)<(.*), (\d+)>\(", name)
        if m and (m.group(1), m.group(2)) in fam:
            d.setdefault((int(m.group(3)), fam[(m.group(1), m.group(2))]), []).append(dur / 1e3)
    for c in bands:
        cp = 4 if c == 3 else 8 if c <= 8 else 16
        mb = {k: v * B / 1e6 for k, v in edge_bytes(c).items()}
        res = {k: {"us": round(statistics.median(d[(cp, k)]), 1), "MB": round(mb[k], 1),
                   "hbm_frac": round(mb[k] / (statistics.median(d[(cp, k)]) * HBM_GBS / 1e3), 3)} for k in mb if (cp, k) in d}
        print(json.dumps({"bands": c, "in_step": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", type=int, nargs="+", default=[3, 4, 8, 13, 16])
    ap.add_argument("--sites", type=int, nargs="*", default=[3, 13])
    ap.add_argument("--no-sites", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prof-db", default=None)
    a = ap.parse_args()
    if a.prof_db:
        prof_db(a.prof_db, a.bands)
        return
    for c in a.bands:
        print(json.dumps(run(c, a.steps, a.warmup)), flush=True)
    if not a.no_sites:
        for c in a.sites:
            print(json.dumps(sites(c)), flush=True)


if __name__ == "__main__":
    main()
