#!/usr/bin/env python3
"""Time of the MLP classifier's kernels per architecture: µs per fused train step at B = 64 and per eval pass over 512 rows, for
    default/fixed      hidden (128, 64), dropout (0.3, 0) on the fixed kernel (eae_mlp_create)
    default/table      the same classifier on the layer-table kernel (eae_mlp_create_ex), alternating with the fixed one
    256x128x64         hidden (256, 128, 64), dropout (0.5, 0.3, 0)
    512x512            hidden (512, 512), dropout (0.3, 0.3)
input_dim 64, 10 classes.  All arms alternate inside one process after --warmup rounds; a repetition is a window of calls between
device events, ending in a synchronise: at least --iters calls, and as many as fill --window-ms (calibrated per arm and call in the
first warm-up round, so a 41 µs eval pass is timed over thousands of calls, not over 8 ms); median, min and max per call over --reps.
The eval logits of the two default arms are compared first: the tool stops with an error unless they are bitwise equal.  A train step
is one launch of one workgroup; the eval pass is one launch over all rows.

    python tools/mlp_arch_bench.py [--reps 9] [--warmup 3] [--iters 200] [--window-ms 300]   ->  one JSON line per arm
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd.mlp_engine import MLPEngine  # noqa: E402

IN, CLASSES, B_TRAIN, B_EVAL = 64, 10, 64, 512
ARMS = [("default/fixed", (128, 64), (0.3, 0.0), False), ("default/table", (128, 64), (0.3, 0.0), True),
        ("256x128x64", (256, 128, 64), (0.5, 0.3, 0.0), None), ("512x512", (512, 512), (0.3, 0.3), None)]


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # µs per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mlp_arch_bench needs the GPU: a time taken elsewhere says nothing")
    g = torch.Generator().manual_seed(0)
    xt, yt = torch.randn(B_TRAIN, IN, generator=g).cuda(), torch.randint(0, CLASSES, (B_TRAIN,), generator=g).cuda()
    xe, ye = torch.randn(B_EVAL, IN, generator=g).cuda(), torch.randint(0, CLASSES, (B_EVAL,), generator=g).cuda()
    engines = []
    for name, hidden, dropout, general in ARMS:
        torch.manual_seed(1)
        clf = eae_amd.MLP(IN, num_classes=CLASSES, hidden=hidden, dropout=dropout).cuda()
        engines.append((name, clf, MLPEngine(clf, max_batch=B_EVAL, general=general)))
    with torch.no_grad():
        if not torch.equal(engines[0][2].forward(xe, train=False), engines[1][2].forward(xe, train=False)):
            sys.exit("the eval logits of the default architecture differ between the fixed and the layer-table kernel")
    calls = {"train_us": lambda e: e.train_step(xt, yt, 1e-3), "eval_us": lambda e: e.eval_step(xe, ye)}
    times = {(name, k): [] for name, _, _ in engines for k in calls}
    iters = {}
    for r in range(args.warmup + args.reps):
        for k, call in calls.items():
            for name, _, eng in engines:
                if r == 0:
                    iters[name, k] = max(args.iters, int(args.window_ms * 1e3 / _timed(lambda: call(eng), args.iters)) + 1)
                t = _timed(lambda: call(eng), iters[name, k])
                if r >= args.warmup:
                    times[name, k].append(t)
    for name, clf, eng in engines:
        row = {"arm": name, "hidden": list(clf.hidden), "dropout": list(clf.dropout), "kernel": "table" if eng.general else "fixed",
               "params": int(eng.poff[-1]), "reps": args.reps, "default_eval_logits_bitwise_equal": True}
        for k in calls:
            v = times[name, k]
            row[k] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "iters": iters[name, k]}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
