#!/usr/bin/env python3
"""Training batches from a scene: windows/s of a `SceneLoader` epoch (stage_scene_windows straight from the scene, crop="window" and
crop="scene") against the path the parent had: materialise every window into a uint16 [N,C,P,P] dataset on the device, then
`stage_bands` by index over the same schedule.  13 x 2048 x 2048 uint16 scene, P = 64, S = 16 and 64, B = 512, train mode (flip, crop,
Philox noise).  Also reported: the one-off materialisation time and the extra device memory the dataset takes (its bytes, and the
allocator's own difference).

--augment adds four arms with an `eae_amd.Augment` policy on, for both crops: `aug_d4radio_*` (quarter turns, gain, band gain and
offset: the integer path) and `aug_full_*` (those plus a rotation of up to 15 degrees and a scale of 0.9 .. 1.1: the bilinear path).

Every arm walks the same number of batches of the same sizes; the arms alternate inside one process, after a warm-up, and a repetition
times whole epochs (--min-windows per repetition at least) between device events, ending in a synchronise.  Median, min and max of
--reps.  The epoch time includes the host side of every batch (argument checks, the C call); the kernels alone come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/scene_stage_bench.py` run (the stage_kernel instantiations of csrc/eae_stage.hip).

    python tools/scene_stage_bench.py [--reps 7] [--warmup 2] [--strides 16 64] [--augment]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402

C, SIZE, P, B = 13, 2048, 64, 512
DIV = 10000.0


def _materialise(scene, stride):
    """uint16 [N,C,P,P]: every window of the grid, in window order (a strided view of the scene, copied)."""
    v = scene.view(torch.int16).unfold(1, P, stride).unfold(2, P, stride)          # [C,nH,nW,P,P]
    return v.permute(1, 2, 0, 3, 4).reshape(-1, C, P, P).contiguous().view(torch.uint16)


def _timed(fn, epochs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(epochs):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / epochs


AUG_ARMS = {"aug_d4radio": dict(dihedral=True, gain=0.2, band_gain=0.1, offset=0.05),
            "aug_full": dict(dihedral=True, rotate=15.0, scale=0.1, gain=0.2, band_gain=0.1, offset=0.05)}


def bench(stride, reps, warmup, min_windows, augment=False, draw_mode=0):
    g = torch.Generator().manual_seed(stride)
    scene = torch.randint(0, 10000, (C, SIZE, SIZE), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    n_h, n_w = eae_amd.window_grid(SIZE, SIZE, P, stride)
    n = n_h * n_w
    label = torch.zeros((n_h, n_w), dtype=torch.int64, device="cuda")
    loaders = {crop: eae_amd.SceneLoader(scene, label, divisor=DIV, patch=P, stride=stride, batch_size=B, crop=crop, seed=1)
               for crop in ("window", "scene")}
    if augment:
        for name, pol in AUG_ARMS.items():
            for crop in ("window", "scene"):
                loaders[f"{name}_{crop}"] = eae_amd.SceneLoader(scene, label, divisor=DIV, patch=P, stride=stride, batch_size=B, crop=crop,
                                                                seed=1, augment=eae_amd.Augment(_draw_mode=draw_mode, **pol))
    sink = torch.zeros((), device="cuda")

    def loader_epoch(crop):
        def fn():
            for x, y in loaders[crop]:
                sink.add_(x[0, 0, 0, 0])                     # the batch is used; nothing is read back
        return fn

    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    data = _materialise(scene, stride)
    b.record()
    b.synchronize()
    mat_s = a.elapsed_time(b) / 1e3
    extra = torch.cuda.memory_allocated() - m0
    assert data.shape == (n, C, P, P) and data.dtype == torch.uint16
    ids = loaders["window"].windows
    epoch = [0]

    def dataset_epoch():
        e = epoch[0]
        epoch[0] += 1
        sched = loaders["window"].schedule(e)
        order = ids[torch.cat(sched).pin_memory().to("cuda", non_blocking=True)]
        at = 0
        for i, s in enumerate(sched):
            x = eae_amd.stage_bands(data, DIV, index=order[at:at + s.numel()], train=True, seed=1, step=e * len(sched) + i)
            sink.add_(x[0, 0, 0, 0])
            at += s.numel()

    # the two paths stage the same batch (crop="window" is bitwise stage_bands on the materialised windows)
    x_l, _ = next(iter(eae_amd.SceneLoader(scene, label, divisor=DIV, patch=P, stride=stride, batch_size=B, seed=1)))
    first = ids[loaders["window"].schedule(0)[0].cuda()]
    assert torch.equal(x_l, eae_amd.stage_bands(data, DIV, index=first, train=True, seed=1, step=0))

    arms = {"loader_window": loader_epoch("window"), "loader_scene": loader_epoch("scene"), "dataset_stage_bands": dataset_epoch}
    for key in loaders:
        if key not in ("window", "scene"):
            arms[key] = loader_epoch(key)
    epochs = max(1, -(-min_windows // n))
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():                           # alternating
            ts[k].append(_timed(fn, epochs))
    res = {"bench": "scene_stage", "scene": [C, SIZE, SIZE], "dtype": "uint16", "patch": P, "stride": stride, "batch": B, "windows": n,
           "batches_per_epoch": len(loaders["window"]), "epochs_per_rep": epochs, "reps": reps,
           "scene_bytes": scene.numel() * 2, "dataset_bytes": data.numel() * 2, "dataset_extra_allocated_bytes": extra,
           "materialise_s": round(mat_s, 5)}
    if augment:
        res["draw_mode"] = draw_mode
    for k, v in ts.items():
        v.sort()
        med = v[len(v) // 2]
        res[k] = {"epoch_s": round(med, 6), "min_s": round(v[0], 6), "max_s": round(v[-1], 6), "windows_per_s": round(n / med, 1)}
    del data, scene
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--strides", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--min-windows", type=int, default=16384, help="windows timed per repetition at least (whole epochs)")
    ap.add_argument("--augment", action="store_true", help="add the arms with an augmentation policy on (both crops)")
    ap.add_argument("--draw-mode", type=int, default=0, choices=[0, 1, 2],
                    help="with --augment: where the per-image draws are made (0: the library's choice, 1: every thread, 2: LDS)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_stage_bench needs a GPU: nothing is measured without one")
    for s in a.strides:
        print(json.dumps(bench(s, a.reps, a.warmup, a.min_windows, a.augment, a.draw_mode)), flush=True)


if __name__ == "__main__":
    main()
