#!/usr/bin/env python3
"""Cost of the global gradient-norm clipping (eae_set_grad_clip) in the joint train step: ms per step with the feature off, with
max_norm = inf (the norm is measured, nothing is clipped) and with a finite max_norm that clips on every step, at B = 512 (one engine,
eae_ae_train_step) and at B = 64 with a group of 8 (eae_group_train_step).

The three arms alternate inside one process on the SAME engines (the setting is switched between blocks of steps), after a warm-up of
all of them; a repetition times --steps steps between device events and ends in a synchronise.  With the feature on a step carries one
launch more on its main chain (the sum-of-squares kernel in front of the optimizer kernel).  Median, min and max of --reps per arm,
and the ratios of the medians to the "off" arm; the "clip" arm also reports the last coefficient (it must be below 1).

    python tools/grad_clip_bench.py [--reps 7] [--steps 100] [--warmup 30]   ->  JSON lines
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
from eae_amd.engine import AEEngine, engine_for  # noqa: E402

ARMS = (("off", None), ("inf", float("inf")), ("clip", 1e-3))


def _timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def bench(batch, group, reps, steps, warmup):
    g = torch.Generator().manual_seed(batch)
    x = torch.rand((batch, 3, 64, 64), generator=g).cuda()
    y = torch.randint(0, 10, (batch,), generator=g).cuda()
    es = []
    for i in range(group):
        torch.manual_seed(100 + i)
        m = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=10).cuda().train()
        if group > 1:
            m._eae_side_streams = 2          # what train.fit_autoencoder_group builds
        es.append(engine_for(m, max_batch=batch))

    def arm(max_norm):
        for e in es:
            e.set_grad_clip(max_norm)
        if group == 1:
            return lambda: es[0].train_step(x, y, 35.0, 1e-3)
        xs, ys, al, lr = [x] * group, [y] * group, [35.0] * group, [1e-3] * group
        return lambda: AEEngine.group_train_step(es, xs, ys, al, lr)

    for _, mn in ARMS:
        fn = arm(mn)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in ARMS}
    coef = None
    for _ in range(reps):
        for name, mn in ARMS:
            ms[name].append(_timed(arm(mn), steps))
            if name == "clip":
                coef = max(e.read_grad_norm()[1] for e in es)
    bad = sum(1 for e in es if e.gate_timeouts())
    out = {"batch": batch, "group": group, "steps": steps, "reps": reps, "gate_timeouts": bad, "clip_coef_max": coef}
    for name, _ in ARMS:
        out[name + "_ms"] = {"median": statistics.median(ms[name]), "min": min(ms[name]), "max": max(ms[name])}
    for name in ("inf", "clip"):
        out[name + "_over_off"] = out[name + "_ms"]["median"] / out["off_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench needs a HIP device")
    for batch, group in ((512, 1), (64, 8)):
        print(json.dumps(bench(batch, group, a.reps, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
