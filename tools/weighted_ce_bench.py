#!/usr/bin/env python3
"""Cost of the class-weighted cross-entropy with ignored labels (eae_set_class_weights) in the joint train step: ms per step with
the feature off and on, at B = 512 (one engine, eae_ae_train_step) and at B = 64 with a group of 8 (eae_group_train_step).

The two arms alternate inside one process on the SAME engines (the setting is switched between blocks of steps), after a warm-up of
both; a repetition times --steps steps between device events and ends in a synchronise.  With the feature on a quarter of the labels
are -1 (ignore_index = -1) and the weights are those of `scene.class_weights(labels, "balanced")`; the labelled-sample count is
part of the "on" arm (the head kernel writes it: no launch of its own).  Median, min and max of --reps per arm, and the
ratio of the medians.  The kernels alone (head_kernel_wce* against head_kernel*) come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/weighted_ce_bench.py` run.

    python tools/weighted_ce_bench.py [--reps 7] [--steps 100] [--warmup 30]   ->  JSON lines
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
    y_off = torch.randint(0, 10, (batch,), generator=g)
    y_on = y_off.clone()
    y_on[torch.rand(batch, generator=g) < 0.25] = -1
    w = eae_amd.class_weights(y_on, 10)
    y_off, y_on = y_off.cuda(), y_on.cuda()
    engs = []
    for i in range(group):
        torch.manual_seed(100 + i)
        m = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=10).cuda().train()
        if group > 1:
            m._eae_side_streams = 2          # what train.fit_autoencoder_group builds
        engs.append((m, engine_for(m, max_batch=batch)))
    es = [e for _, e in engs]

    def arm(on):
        for e in es:
            e.set_class_weights(w if on else None, -1 if on else None)
        y = y_on if on else y_off
        if group == 1:
            return lambda: es[0].train_step(x, y, 35.0, 1e-3)
        xs, ys, al, lr = [x] * group, [y] * group, [35.0] * group, [1e-3] * group
        return lambda: AEEngine.group_train_step(es, xs, ys, al, lr)

    for on in (False, True):
        fn = arm(on)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            ms[on].append(_timed(arm(on), steps))
    bad = sum(1 for e in es if e.gate_timeouts())
    out = {"batch": batch, "group": group, "steps": steps, "reps": reps, "gate_timeouts": bad}
    for on, name in ((False, "off"), (True, "on")):
        out[name + "_ms"] = {"median": statistics.median(ms[on]), "min": min(ms[on]), "max": max(ms[on])}
    out["on_over_off"] = out["on_ms"]["median"] / out["off_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weighted_ce_bench needs a HIP device")
    for batch, group in ((512, 1), (64, 8)):
        print(json.dumps(bench(batch, group, a.reps, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
