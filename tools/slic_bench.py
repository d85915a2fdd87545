#!/usr/bin/env python3
"""One SLIC iteration on the device: `eae_slic_step` (assignment and accumulation fused, one pass over the scene; integer tables)
against two references measured in the same process on the same machine:

    torch     the same iteration in torch (quantise in float64, gather the nine candidate centres of every pixel, int64 D, argmin,
              `index_add_` of the C + 3 columns), at --torch-size (it does not fit at 8192^2), asserted equal to the kernel there;
    copy      a plain device copy of the scene's bytes, the streaming floor of a pass that reads the scene once.

Workloads: 8192^2 x 4 bands uint16 at step 16 and step 64, 8192^2 x 3 bands uint8 at step 16 (blocks of 48 pixels of one colour
with noise).  The timed step is iteration 3 of a run (centres that have moved), without the label write, and again with it (the
last iteration of `slic_clusters`).  The whole `slic_scene` at 10 iterations (its sieve, regions and compaction included) is timed
beside them.  The arms alternate after --warmup rounds; a repetition is one call between device events, ending in a synchronise;
median, min and max of --reps.  TB/s counts the scene's bytes, the bytes the algorithm has to read (plus the int32 labels where
they are written); for the copy, the bytes copied (read once and written once).  Peak extra memory is
`torch.cuda.max_memory_allocated` over one call less what was allocated before it: for `eae_slic_step` the caller's sums table,
since the call allocates nothing.  The kernel alone comes from a separate `rocprofv3 --kernel-trace --stats -- python
tools/slic_bench.py` run (slic_step_kernel).

    python tools/slic_bench.py [--reps 7] [--warmup 2] [--size 8192] [--torch-size 2048] [--no-scene]   ->  JSON lines
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eae_amd  # noqa: E402
from eae_amd import _lib  # noqa: E402
from eae_amd.engine import _ptr, _stream  # noqa: E402
from eae_amd.segment import spatial_weight  # noqa: E402

DTYPE_ID = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}
WORKLOADS = ((4, torch.uint16, 16), (4, torch.uint16, 64), (3, torch.uint8, 16))


def make_scene(c, size, dtype, g):
    top = 255 if dtype == torch.uint8 else 65535
    coarse = torch.randint(top // 8, top - top // 8, (c, -(-size // 48), -(-size // 48)), generator=g, device="cuda")
    s = coarse.repeat_interleave(48, 1).repeat_interleave(48, 2)[:, :size, :size]
    s = s + torch.randint(-(top // 40), top // 40 + 1, (c, size, size), generator=g, device="cuda")
    return s.clamp_(0, top).to(dtype if dtype == torch.uint8 else torch.int32).to(dtype)


class Step:
    """`eae_slic_step` + `eae_slic_centres` on preallocated tables."""

    def __init__(self, scene, div, step, weight):
        self.scene, self.div, self.step, self.weight = scene, div, step, weight
        c, h, w = scene.shape
        self.n_cl = (-(-h // step)) * (-(-w // step))
        self.sums = torch.empty((self.n_cl, c + 3), dtype=torch.int64, device=scene.device)
        self.centres = torch.empty((self.n_cl, c + 3), dtype=torch.int32, device=scene.device)
        self.labels = torch.empty((h, w), dtype=torch.int32, device=scene.device)
        self.lib = _lib.load()

    def run(self, centres, labels=False):
        c, h, w = self.scene.shape
        _lib.check(self.lib.eae_slic_step(_stream(), _ptr(self.scene), DTYPE_ID[self.scene.dtype], c, h, w, _ptr(self.div), None,
                                          self.step, self.weight, _ptr(centres), _ptr(self.sums), _ptr(self.labels) if labels else None))

    def update(self):
        _lib.check(self.lib.eae_slic_centres(_stream(), _ptr(self.sums), self.n_cl, self.scene.shape[0], _ptr(self.centres)))


def torch_step(scene, div, step, weight, centres):
    """The same iteration in torch: (labels int64 [H, W], sums int64 [n_cl, C + 3])."""
    c, h, w = scene.shape
    n_h, n_w = -(-h // step), -(-w // step)
    p = scene.to(torch.float64) / div.to(torch.float64).reshape(c, 1, 1)
    u = torch.round(65535.0 * torch.where(p > 0, torch.where(p < 1, p, 1.0), 0.0)).to(torch.int64)
    y = torch.arange(h, device=scene.device)[:, None].expand(h, w)
    x = torch.arange(w, device=scene.device)[None, :].expand(h, w)
    hi, hj = y // step, x // step
    cen = centres.to(torch.int64)
    best = torch.full((h, w), 2 ** 63 - 1, dtype=torch.int64, device=scene.device)
    labels = torch.full((h, w), -1, dtype=torch.int64, device=scene.device)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            i, j = hi + di, hj + dj
            inside = (i >= 0) & (i < n_h) & (j >= 0) & (j < n_w)
            k = torch.where(inside, i * n_w + j, 0)
            row = cen[k]                                              # the gather: [H, W, C + 3]
            ok = inside & (row[..., 0] > 0)
            colour = ((u.permute(1, 2, 0) - row[..., 3:]) ** 2).sum(-1)
            dy, dx = torch.where(ok, y - row[..., 1], 0), torch.where(ok, x - row[..., 2], 0)
            d = step * step * colour + weight * (dy * dy + dx * dx)
            take = ok & (d < best)
            best = torch.where(take, d, best)
            labels = torch.where(take, k, labels)
    cols = torch.cat([torch.ones((1, h, w), dtype=torch.int64, device=scene.device), y[None], x[None], u]).reshape(c + 3, -1).t()
    sums = torch.zeros((n_h * n_w, c + 3), dtype=torch.int64, device=scene.device)
    sums.index_add_(0, labels.reshape(-1), cols.contiguous())
    return labels, sums


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def _stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def _warm_centres(st):
    """Three iterations: centres that have moved off the grid."""
    st.run(None)
    st.update()
    for _ in range(2):
        st.run(st.centres)
        st.update()
    return st.centres.clone()


def bench(c, dtype, step, size, tsize, reps, warmup, with_scene):
    g = torch.Generator(device="cuda").manual_seed(size + step)
    scene = make_scene(c, size, dtype, g)
    small = scene[:, :tsize, :tsize].contiguous()
    div = torch.full((c,), 255.0 if dtype == torch.uint8 else 65535.0, device="cuda")
    weight = spatial_weight(0.1)
    st, ss = Step(scene, div, step, weight), Step(small, div, step, weight)
    cen, cen_s = _warm_centres(st), _warm_centres(ss)
    # the torch formulation and the kernel agree at the size the former fits
    ss.run(cen_s, labels=True)
    tl, ts_ = torch_step(small, div, step, weight, cen_s)
    assert torch.equal(ss.labels.to(torch.int64), tl) and torch.equal(ss.sums, ts_), "the torch formulation and the kernel disagree"
    del tl, ts_
    st.run(cen)
    first = st.sums.clone()
    st.run(cen)
    assert torch.equal(st.sums, first) and int(first[:, 0].sum()) == size * size, "two runs differ"
    del first
    copy_dst = torch.empty_like(scene)
    arms = {"slic_step": lambda: st.run(cen), "slic_step_labels": lambda: st.run(cen, labels=True),
            "device_copy": lambda: copy_dst.copy_(scene),
            "slic_step_small": lambda: ss.run(cen_s, labels=True), "torch_step_small": lambda: torch_step(small, div, step, weight, cen_s)}
    if with_scene:
        arms["slic_scene_10"] = lambda: eae_amd.slic_scene(scene, step, 0.1, iterations=10, divisor=div)
    peak = {k: _peak_extra(fn) for k, fn in arms.items()}
    peak["slic_step"] = peak["slic_step_labels"] = st.sums.numel() * 8          # the call allocates nothing: its caller's sums table
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():                           # alternating
            ts[k].append(_timed(fn))
    eb = scene.element_size()
    full, sm = c * size * size * eb, c * tsize * tsize * eb
    nbytes = {"slic_step": full, "slic_step_labels": full + 4 * size * size, "device_copy": full, "slic_step_small": sm + 4 * tsize * tsize,
              "torch_step_small": sm + 4 * tsize * tsize, "slic_scene_10": None}
    res = {"bench": "slic_step", "scene": [c, size, size], "dtype": str(dtype).replace("torch.", ""), "step": step,
           "clusters": st.n_cl, "torch_size": tsize, "reps": reps}
    for k, v in ts.items():
        res[k] = dict(_stats(v), bytes=nbytes[k], peak_extra_bytes=peak[k])
        if nbytes[k]:
            res[k]["tb_per_s"] = round(nbytes[k] / (res[k]["ms"] * 1e-3) / 1e12, 3)
    res["step_over_copy"] = round(res["slic_step"]["ms"] / res["device_copy"]["ms"], 2)
    res["torch_over_step_small"] = round(res["torch_step_small"]["ms"] / res["slic_step_small"]["ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--torch-size", type=int, default=2048)
    ap.add_argument("--no-scene", action="store_true", help="leave the whole slic_scene out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slic_bench needs a GPU: nothing is measured without one")
    for c, dtype, step in WORKLOADS:
        print(json.dumps(bench(c, dtype, step, a.size, min(a.torch_size, a.size), a.reps, a.warmup, not a.no_scene)), flush=True)


if __name__ == "__main__":
    main()
