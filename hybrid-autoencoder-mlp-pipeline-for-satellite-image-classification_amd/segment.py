"""Superpixels on the device: SLIC segmentation of a scene into the zones `classify_zones` takes.

`zonal.py` gives one class per zone of a zone raster; this module makes that raster from the scene itself, so a user with nothing but
a scene on the device can run the object-based chain.  The kernels are those of the C library (include/eae.h, "superpixels";
DESIGN.md section 35).  Everything is integer arithmetic, so clusters, centres and zones are unique for given inputs and identical
from run to run:

- a pixel's feature in band c is u_c = rint(65535 * min(max(v / divisor_c, 0), 1)) (float64, round-half-even, NaN -> 0);
- the grid has ceil(H / step) x ceil(W / step) cells, cluster i * n_w + j starts as cell (i, j);
- an iteration gives every unmasked pixel to the cluster, among the non-empty ones of the 3 x 3 cells around its home cell, with the
  smallest D = step^2 * sum_c (u_c - mu_c)^2 + M * ((y - cy)^2 + (x - cx)^2), the lowest id on a tie, M = rint((65535 *
  compactness)^2); the centres are then the rounded means (2 sum + n) // (2 n) of the new assignment.

- `slic_clusters`: the cluster of every pixel and the centres, no read-back;
- `slic_scene`: clusters, one sieve pass, connected regions, dense zone ids: a `Superpixels`;
- `classify_superpixels`: `slic_scene`, then `classify_zones` with its zones;
- `zone_boundaries`: the outlines of a zone raster for overlays (plain torch).

Nodata is not handled here: pass ``mask=``.
"""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check
from ._args import _int_arg
from .engine import _ptr, _stream, _require_gpu
from .postprocess import _connectivity_arg, _regions, _stats, _workspace

MIN_STEP, MAX_STEP = 2, 256
MAX_BANDS = 16
MAX_WEIGHT = 2 ** 40
_INT_MAX = 2 ** 31 - 1
_PIXEL_LIMIT = 2 ** 31
U_ONE = 65535                 # the quantised feature of a value equal to its divisor


class Superpixels(NamedTuple):
    """zones int32 [H, W]: dense ids 0 .. num_zones - 1 of connected zones, -1 for a masked pixel; num_zones; clusters int32 [H, W]:
    the SLIC cluster of every pixel before the sieve; centres int32 [n_clusters, C + 3] = (count, cy, cx, mu_0, ..)."""
    zones: torch.Tensor
    num_zones: int
    clusters: torch.Tensor
    centres: torch.Tensor


class _Args(NamedTuple):
    scene: torch.Tensor
    div: torch.Tensor            # fp32 [C], wherever the caller's divisor was
    mask: object                 # uint8 [H, W] or None
    step: int
    weight: int                  # M
    iterations: int
    n_h: int
    n_w: int


# ---------------------------------------------------------------------------------------------------- host-side validation
def spatial_weight(compactness):
    """M = rint((65535 * compactness)^2) in float64: the weight of a squared pixel distance against a squared feature distance."""
    if isinstance(compactness, bool) or not isinstance(compactness, numbers.Real) or not math.isfinite(float(compactness)) \
            or float(compactness) < 0.0:
        raise RuntimeError(f"compactness must be a finite number >= 0, got {compactness!r}")
    m = int(round((float(U_ONE) * float(compactness)) ** 2))           # round(): half-even on a float, as rint
    if m > MAX_WEIGHT:
        raise RuntimeError(f"compactness {compactness!r} gives a spatial weight of {m}: it must stay in 0..2^40 (compactness <= 16)")
    return m


def _host_args(scene, step, compactness, iterations, divisor, mask):
    """Every host-side check of the SLIC functions; no device is touched."""
    from .scene import _check_scene, _mask_arg
    _check_scene(scene)
    c, h, w = (int(v) for v in scene.shape)
    if not 1 <= c <= MAX_BANDS:
        raise RuntimeError(f"scene: the number of bands must be in 1..16, got {c}")
    if h < 1 or w < 1:
        raise RuntimeError(f"scene is empty: {[c, h, w]}")
    if h * w >= _PIXEL_LIMIT:
        raise RuntimeError(f"scene has {h} x {w} pixels: H * W must be below 2^31")
    step = _int_arg(step, "step", MIN_STEP, MAX_STEP)
    weight = spatial_weight(compactness)
    iterations = _int_arg(iterations, "iterations", 1, _INT_MAX)
    n_h, n_w = -(-h // step), -(-w // step)
    if n_h * n_w * (c + 3) > _INT_MAX:
        raise RuntimeError(f"step {step} gives {n_h} x {n_w} clusters: n_h * n_w * (C + 3) must not exceed 2^31 - 1")
    div = torch.as_tensor(divisor, dtype=torch.float32).reshape(-1)
    if div.numel() == 1:
        div = div.expand(c)
    if div.numel() != c:
        raise RuntimeError(f"divisor must have one value per band ({c}), got {div.numel()}")
    return _Args(scene, div, _mask_arg(scene, mask), step, weight, iterations, n_h, n_w)


def _min_size_arg(min_size, step):
    if min_size is None:
        return max(1, step * step // 4)
    return _int_arg(min_size, "min_size", 1, 2 ** 63 - 1)


# ---------------------------------------------------------------------------------------------------- slic_clusters
def _clusters(a):
    """(labels int32 [H, W], centres int32 [n_cl, C + 3]) of checked arguments: the initialisation, then ``iterations`` steps of which
    only the last writes labels.  Two sums / centres tables and the label raster are all the memory the iteration takes."""
    from .scene import _DTYPES
    _require_gpu(a.scene.device)
    scene = a.scene.contiguous()
    dev = scene.device
    c, h, w = (int(v) for v in scene.shape)
    div = a.div.to(dev).contiguous()
    n_cl = a.n_h * a.n_w
    sums = torch.empty((n_cl, c + 3), dtype=torch.int64, device=dev)
    centres = torch.empty((n_cl, c + 3), dtype=torch.int32, device=dev)
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        for it in range(a.iterations + 1):
            last = it == a.iterations
            check(lib.eae_slic_step(_stream(), _ptr(scene), _DTYPES[scene.dtype], c, h, w, _ptr(div), _ptr(a.mask), a.step, a.weight,
                                    _ptr(centres) if it else None, _ptr(sums), _ptr(labels) if last else None))
            check(lib.eae_slic_centres(_stream(), _ptr(sums), n_cl, c, _ptr(centres)))
    return labels, centres


def slic_clusters(scene, step, compactness=0.1, iterations=10, divisor=1.0, mask=None):
    """(labels int32 [H, W], centres int32 [n_clusters, C + 3]) on the device, nothing read back.  ``scene`` [C, H, W]: uint8, uint16
    or float32, C in 1..16; ``divisor``: a number or one per band, as the scene functions take it; ``mask``: None or bool / uint8
    [H, W], non-zero = the pixel takes no part (label -1).  ``step`` in 2..256 is the grid spacing, ``compactness`` weighs space
    against colour (0: colour only; it must keep M = rint((65535 * compactness)^2) within 2^40), and ``iterations`` >= 1 steps run
    after the initialisation.  The centres are those of the returned labels: (count, cy, cx, mu_0, ..), an empty cluster all zeros."""
    return _clusters(_host_args(scene, step, compactness, iterations, divisor, mask))


# ---------------------------------------------------------------------------------------------------- slic_scene
def _zones_of(clusters, min_size, connectivity):
    """(zones int32 [H, W], Z) from the cluster raster: one sieve pass over the regions of equal cluster, the connected regions of the
    result, dense ids in ascending order of a region's smallest linear index.  The read-back is Z."""
    from .zonal import compact_zones
    h, w = clusters.shape
    src = clusters.to(torch.int64)
    lib = _lib.load()
    with torch.cuda.device(src.device):
        ws = _workspace(h, w, src.device)
        regions = _regions(src, None, connectivity, ws)
        area, _ = _stats(regions, False)
        sieved = torch.empty_like(src)
        check(lib.eae_map_sieve_pass(_stream(), _ptr(src), _ptr(regions), _ptr(area), h, w, min_size, _ptr(sieved), None, _ptr(ws),
                                     ws.numel()))
        regions = _regions(sieved, None, connectivity, ws)
    zones, ids = compact_zones(regions)
    return zones, int(ids.numel())


def slic_scene(scene, step, compactness=0.1, iterations=10, divisor=1.0, mask=None, min_size=None, connectivity=4):
    """`Superpixels` of a scene: `slic_clusters`, then one `sieve` pass over the clusters at ``connectivity`` (4 or 8) with threshold
    ``min_size`` (default max(1, step^2 // 4)), the connected regions of the sieved clusters, and `compact_zones`.  A zone is
    therefore always connected; a large detached fragment of a cluster becomes a zone of its own.  Masked pixels are -1 in ``zones``
    and ``clusters``.  One read-back: the number of zones."""
    a = _host_args(scene, step, compactness, iterations, divisor, mask)
    min_size = _min_size_arg(min_size, a.step)
    connectivity = _connectivity_arg(connectivity)
    clusters, centres = _clusters(a)
    zones, z = _zones_of(clusters, min_size, connectivity)
    return Superpixels(zones, z, clusters, centres)


# ---------------------------------------------------------------------------------------------------- classify_superpixels
def classify_superpixels(scene, encoder, mlp, step, compactness=0.1, iterations=10, min_size=None, connectivity=4, rule="probs",
                         min_coverage=0.5, divisor=1.0, stride=None, batch=512, blend=False, nodata=None, mask=None, max_invalid=0.0,
                         invalid_rule="all", windows=None, border=None, fill=0, anchor="center"):
    """`slic_scene` of the scene, then `classify_zones` with its zones: one class per superpixel and the map painted back.  The
    arguments up to ``connectivity`` are `slic_scene`'s, the rest `classify_zones`'s; ``divisor`` and ``mask`` go to both (``nodata``
    only decides which windows are classified: mask such pixels to keep them out of the segmentation).  Returns the `classify_zones`
    dict plus ``"superpixels"``: the `Superpixels`."""
    from .scene import _host_plan
    from .zonal import classify_zones, _rule_arg, _coverage_arg
    a = _host_args(scene, step, compactness, iterations, divisor, mask)
    min_size = _min_size_arg(min_size, a.step)
    connectivity = _connectivity_arg(connectivity)
    # classify_zones' own host checks, before the segmentation spends time on the device
    _rule_arg(rule)
    _coverage_arg(min_coverage)
    _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, invalid_rule, windows, blend=blend, border=border,
               fill=fill, anchor=anchor, mlp=mlp)
    clusters, centres = _clusters(a)
    zones, z = _zones_of(clusters, min_size, connectivity)
    out = classify_zones(scene, encoder, mlp, zones, num_zones=max(z, 1), rule=rule, min_coverage=min_coverage, divisor=divisor,
                         stride=stride, batch=batch, blend=blend, nodata=nodata, mask=mask, max_invalid=max_invalid,
                         invalid_rule=invalid_rule, windows=windows, border=border, fill=fill, anchor=anchor)
    out["superpixels"] = Superpixels(zones, z, clusters, centres)
    return out


# ---------------------------------------------------------------------------------------------------- zone_boundaries
def zone_boundaries(zones, connectivity=4):
    """bool [H, W], true where the right or the lower neighbour (with ``connectivity=8`` also the lower-left or lower-right one) holds
    another id: the outlines of a zone raster, one pixel wide, for overlays.  Plain torch, on the raster's device (CPU tensors work)."""
    from .zonal import _zones_arg
    _zones_arg(zones)
    connectivity = _connectivity_arg(connectivity)
    out = torch.zeros(zones.shape, dtype=torch.bool, device=zones.device)
    out[:, :-1] |= zones[:, :-1] != zones[:, 1:]
    out[:-1, :] |= zones[:-1, :] != zones[1:, :]
    if connectivity == 8:
        out[:-1, :-1] |= zones[:-1, :-1] != zones[1:, 1:]
        out[:-1, 1:] |= zones[:-1, 1:] != zones[1:, :-1]
    return out
