"""Object-based classification: one class per zone of a zone raster, from everything the model said inside it.

A zone raster is an integer [H, W] tensor of object ids at the scene's pixel resolution -- field parcels, cadastral polygons, segments,
or the regions `label_regions` computes: an id in [0, num_zones) is a zone, every other id (negatives: "no zone") is skipped.  The
class map is what `classify_scene` and its siblings return: an int64 [cH, cW] map of ``cell`` x ``cell`` cells and, optionally, the
float32 [K, cH, cW] probabilities of the same cells; pixel (y, x) lies in cell ((y + oy) // cell, (x + ox) // cell), as in
`scene_confusion`.  The kernels are those of the C library (include/eae.h, "zonal statistics").

- `compact_zones`: any integer raster (sparse parcel ids, `label_regions` output) to dense ids 0 .. Z-1 and the table back;
- `zonal_stats`: per zone, the pixels that voted for each class and the fixed-point sums of the class probabilities (device);
- `zone_labels`: one label, its confidence and the zone's coverage from those tables (plain torch, device or CPU);
- `paint_zones`: a per-zone value painted back at pixel resolution (device);
- `classify_zones`: `classify_scene`, then the three above: the per-object map of a scene;
- `zone_confusion`: object-level confusion counts, one per zone, for `report.confusion_metrics`.

Everything the device computes here is an integer sum, so it is exact and identical from run to run.  A probability enters a sum as
q(p) = rint(2^32 * min(max(p, 0), 1)) (in float64, round-half-even, NaN -> 0): at most 2^32 per pixel and fewer than 2^31 pixels per
zone, so an int64 sum cannot overflow, and comparing two sums compares integers.
"""
from __future__ import annotations

import numbers
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check
from ._args import _int_arg
from .engine import _ptr, _stream, _require_gpu

MAX_CLASSES = 64
_INT_MAX = 2 ** 31 - 1
_PIXEL_LIMIT = 2 ** 31
Q_ONE = 2 ** 32                 # q(1.0): the fixed-point unit of prob_sums
_RULES = ("probs", "votes")


class ZonalStats(NamedTuple):
    """votes int64 [Z, K+1]: the pixels of zone z whose cell has class c (column K: not classified / not covered);
    prob_sums int64 [Z, K] or None: the sums of q(probs[j]) over the zone's classified pixels."""
    votes: torch.Tensor
    prob_sums: Optional[torch.Tensor]


# ---------------------------------------------------------------------------------------------------- host-side validation
def _is_int_tensor(t):
    return isinstance(t, torch.Tensor) and not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _zones_arg(zones):
    """(H, W) of an integer [H, W] zone raster with H, W >= 1 and H * W < 2^31."""
    if not isinstance(zones, torch.Tensor) or zones.dim() != 2:
        raise RuntimeError("zones must be a [H, W] tensor of zone ids")
    if not _is_int_tensor(zones):
        raise RuntimeError(f"zones must have an integer dtype, got {zones.dtype}")
    h, w = int(zones.shape[0]), int(zones.shape[1])
    if h < 1 or w < 1:
        raise RuntimeError(f"zones is empty: {[h, w]}")
    if h * w >= _PIXEL_LIMIT:
        raise RuntimeError(f"zones has {h} x {w} pixels: H * W must be below 2^31")
    return h, w


def _native_zones(zones):
    """The raster as the kernels read it: int32 and int64 pass through (made contiguous), narrower dtypes become int32."""
    if zones.dtype not in (torch.int32, torch.int64):
        zones = zones.to(torch.int32)
    return zones.contiguous()


def _num_zones_arg(z, k=0):
    z = _int_arg(z, "num_zones", 1, _INT_MAX)
    if z * (k + 1) > _INT_MAX:
        raise RuntimeError(f"num_zones * (num_classes + 1) must not exceed 2^31 - 1, got {z} * {k + 1}")
    return z


def _stats_arg(stats, what="stats"):
    """(Z, K) of a `ZonalStats` whose tables agree."""
    if not isinstance(stats, ZonalStats):
        raise RuntimeError(f"{what} must be a ZonalStats (what zonal_stats returns), got {type(stats).__name__}")
    v, p = stats.votes, stats.prob_sums
    if not isinstance(v, torch.Tensor) or v.dtype != torch.int64 or v.dim() != 2 or v.shape[1] < 2 or v.shape[0] < 1:
        raise RuntimeError(f"{what}.votes must be an int64 [Z, K+1] tensor")
    z, k = int(v.shape[0]), int(v.shape[1]) - 1
    if p is not None and (not isinstance(p, torch.Tensor) or p.dtype != torch.int64 or tuple(p.shape) != (z, k) or p.device != v.device):
        raise RuntimeError(f"{what}.prob_sums must be None or an int64 [{z}, {k}] tensor on the device of votes")
    return z, k


# ---------------------------------------------------------------------------------------------------- compact_zones
def compact_zones(ids):
    """(zones int32 [H, W], ids int64 [Z]): the distinct non-negative values of an integer raster numbered 0 .. Z-1 in ascending
    order, negatives -> -1; ``ids[zones[y, x]]`` is the value the pixel held.  For `label_regions` output (sparse linear indices) and
    sparse parcel ids.  `torch.unique` plumbing: works on CPU tensors too; one read-back for Z.  A raster without a non-negative
    value has no zone: Z = 0 and every pixel -1.  The device calls take at least one zone (``num_zones >= 1``, a non-empty
    ``values``), so pass ``max(len(ids), 1)`` where that can happen: the one zone stays empty, which is what `classify_zones` does
    for such a raster."""
    _zones_arg(ids)
    values, inverse = torch.unique(ids, return_inverse=True)          # ascending: the negatives come first
    negatives = (values < 0).sum()
    zones = torch.where(ids < 0, -1, inverse - negatives).to(torch.int32)
    return zones, values[values >= 0].to(torch.int64)


# ---------------------------------------------------------------------------------------------------- zonal_stats
def zonal_stats(zones, num_zones, labels, num_classes, probs=None, cell=1, origin=(0, 0), mask=None, out=None):
    """`ZonalStats` (on the device) of a class map inside every zone.  ``zones`` [H, W]: zone ids of any integer dtype (int32 and
    int64 are read as they are, narrower dtypes are converted to int32); ``labels``: an integer [cH, cW] map of ``cell`` x ``cell``
    cells; ``probs``: None or the float32 [K, cH, cW] probabilities of the same cells; ``mask``: None or bool / uint8 [H, W].

    Every pixel (y, x) with ``mask[y, x] == 0`` and z = zones[y, x] in [0, num_zones) lies in cell ((y + oy) // cell, (x + ox) //
    cell), (oy, ox) = ``origin``; c = the cell's label when the cell lies inside the map and the label is in [0, K), else K.  Then
    votes[z, c] += 1 and, with ``probs`` and c < K, prob_sums[z, j] += q(probs[j, cell]) for every class j (q: module docstring).
    ``out=``: an earlier result to add to (several scenes), with prob_sums exactly when ``probs`` is given.

    cell=1 against a raster of the map's own shape covers `label_regions` output and per-zone truth from a label raster.  Exact
    integer sums: identical from run to run."""
    k = _int_arg(num_classes, "num_classes", 1, MAX_CLASSES)
    h, w = _zones_arg(zones)
    z = _num_zones_arg(num_zones, k)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or not _is_int_tensor(labels):
        raise RuntimeError("labels must be a 2-D integer map of class ids")
    c_h, c_w = int(labels.shape[0]), int(labels.shape[1])
    if min(c_h, c_w) < 1:
        raise RuntimeError(f"labels is empty: {[c_h, c_w]}")
    if max(c_h, c_w) > _INT_MAX:
        raise RuntimeError("labels is too large")
    if labels.device != zones.device:
        raise RuntimeError(f"labels is on {labels.device}, zones on {zones.device}")
    if probs is not None:
        if not isinstance(probs, torch.Tensor) or probs.dtype != torch.float32 or tuple(probs.shape) != (k, c_h, c_w):
            got = f"{probs.dtype} {list(probs.shape)}" if isinstance(probs, torch.Tensor) else type(probs).__name__
            raise RuntimeError(f"probs must be a float32 [K, cH, cW] = {[k, c_h, c_w]} tensor, got {got}")
        if probs.device != zones.device:
            raise RuntimeError(f"probs is on {probs.device}, zones on {zones.device}")
    if isinstance(cell, bool) or not isinstance(cell, numbers.Integral) or not 1 <= int(cell) <= _INT_MAX:
        raise RuntimeError(f"cell must be a positive integer, got {cell!r}")
    cell = int(cell)
    try:
        oy, ox = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise RuntimeError(f"origin must be a pair (oy, ox) of integers, got {origin!r}") from None
    if not (0 <= oy <= _INT_MAX and 0 <= ox <= _INT_MAX):
        raise RuntimeError(f"origin must not be negative, got {origin!r}")
    from .scene import _mask_arg
    m = _mask_arg(zones.unsqueeze(0), mask)
    if out is not None:
        oz, ok = _stats_arg(out, "out")
        if (oz, ok) != (z, k) or (out.prob_sums is None) != (probs is None):
            raise RuntimeError(f"out must hold votes [{z}, {k + 1}] and prob_sums {'[%d, %d]' % (z, k) if probs is not None else 'None'} "
                               "(an earlier result of the same call)")
        if out.votes.device != zones.device or not out.votes.is_contiguous() or (probs is not None and not out.prob_sums.is_contiguous()):
            raise RuntimeError(f"out must be contiguous and on {zones.device}")
    _require_gpu(zones.device)
    zones = _native_zones(zones)
    labels = labels.to(torch.int64).contiguous()
    probs = None if probs is None else probs.contiguous()
    if out is None:
        votes = torch.empty((z, k + 1), dtype=torch.int64, device=zones.device)
        sums = None if probs is None else torch.empty((z, k), dtype=torch.int64, device=zones.device)
    else:
        votes, sums = out.votes, out.prob_sums
    lib = _lib.load()
    with torch.cuda.device(zones.device):
        check(lib.eae_zonal_accumulate(_stream(), _ptr(zones), zones.element_size(), h, w, _ptr(labels), _ptr(probs), c_h, c_w, cell, oy,
                                       ox, _ptr(m), k, z, int(out is not None), _ptr(votes), _ptr(sums)))
    return out if out is not None else ZonalStats(votes, sums)


# ---------------------------------------------------------------------------------------------------- zone_labels
def _rule_arg(rule):
    if rule not in _RULES:
        raise RuntimeError(f"rule must be 'probs' or 'votes', got {rule!r}")
    return rule


def _coverage_arg(min_coverage):
    if isinstance(min_coverage, bool) or not isinstance(min_coverage, numbers.Real) or not 0.0 <= float(min_coverage) <= 1.0:
        raise RuntimeError(f"min_coverage must be a number in [0, 1], got {min_coverage!r}")
    return float(min_coverage)


def zone_labels(stats, rule="probs", min_coverage=0.0):
    """(label int64 [Z], confidence float32 [Z], coverage float32 [Z]) from a `ZonalStats`, on its device (CPU tensors work too).
    With total = votes.sum(1) and classified = votes[:, :K].sum(1):

    - rule="probs": the class with the largest prob_sums, confidence = that sum / (2^32 * classified), the mean probability of the
      winner over the zone's classified pixels;
    - rule="votes": the class with the most votes, confidence = its votes / classified.

    The lowest class wins a tie, and the comparison is made on the integers: it is exact.  A zone with classified == 0, or with
    classified < min_coverage * total (compared in float64), gets label -1 and confidence NaN.  coverage = classified / total, NaN
    for an empty zone."""
    rule = _rule_arg(rule)
    min_coverage = _coverage_arg(min_coverage)
    _, k = _stats_arg(stats)
    if rule == "probs" and stats.prob_sums is None:
        raise RuntimeError("rule='probs' needs prob_sums: call zonal_stats with probs=, or use rule='votes'")
    votes = stats.votes
    table = stats.prob_sums if rule == "probs" else votes[:, :k]
    total, classified = votes.sum(1), votes[:, :k].sum(1)
    best = table.max(dim=1, keepdim=True).values
    classes = torch.arange(k, dtype=torch.int64, device=votes.device)
    label = torch.where(table == best, classes, k).min(dim=1).values           # the first maximum: the lowest class on a tie
    tot64, cls64 = total.to(torch.float64), classified.to(torch.float64)
    scale = float(Q_ONE) if rule == "probs" else 1.0
    confidence = best[:, 0].to(torch.float64) / (cls64 * scale)
    keep = (classified > 0) & ~(cls64 < min_coverage * tot64)
    label = torch.where(keep, label, -1)
    confidence = torch.where(keep, confidence, float("nan")).to(torch.float32)
    coverage = (cls64 / tot64).to(torch.float32)                               # 0 / 0 = NaN: an empty zone
    return label, confidence, coverage


# ---------------------------------------------------------------------------------------------------- paint_zones
def paint_zones(zones, values, fill=-1):
    """int64 [H, W]: ``values[zones[y, x]]`` where the id is in [0, len(values)), else ``fill`` -- a per-zone label, or any other
    per-zone integer, at pixel resolution.  One pass on the device; the zone raster is read in its own dtype (narrower than int32:
    converted to int32)."""
    h, w = _zones_arg(zones)
    if not isinstance(values, torch.Tensor) or values.dim() != 1 or values.dtype != torch.int64 or values.numel() < 1:
        raise RuntimeError("values must be a non-empty 1-D int64 tensor, one entry per zone")
    if values.device != zones.device:
        raise RuntimeError(f"values is on {values.device}, zones on {zones.device}")
    fill = _int_arg(fill, "fill", -2 ** 63, 2 ** 63 - 1)
    _require_gpu(zones.device)
    zones, values = _native_zones(zones), values.contiguous()
    out = torch.empty((h, w), dtype=torch.int64, device=zones.device)
    with torch.cuda.device(zones.device):
        check(_lib.load().eae_zonal_paint(_stream(), _ptr(zones), zones.element_size(), h, w, _ptr(values), values.numel(), fill,
                                          _ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------------- classify_zones
def classify_zones(scene, encoder, mlp, zones, num_zones=None, rule="probs", min_coverage=0.5, divisor=1.0, stride=None, batch=512,
                   blend=False, nodata=None, mask=None, max_invalid=0.0, invalid_rule="all", windows=None, border=None, fill=0,
                   anchor="center"):
    """One class per zone of a scene, and the map painted back: `classify_scene` with the arguments after ``min_coverage`` (its
    ``rule`` is ``invalid_rule`` here), then `zonal_stats` of its probabilities and labels, `zone_labels` with ``rule`` and
    ``min_coverage``, and `paint_zones`.  The geometry is `evaluate_scene`'s: blend=False needs stride == patch, the cell is the
    stride and the origin the leading pads of the border grid.  ``zones`` [H, W]: zone ids at the scene's size (dense; see
    `compact_zones`); num_zones=None takes ``zones.max() + 1`` (one read-back).  ``mask`` / ``nodata`` decide which windows are
    classified; their pixels count as not classified in their zones.

    Returns {"zone_labels" int64 [Z], "confidence" float32 [Z], "coverage" float32 [Z], "stats": `ZonalStats`, "map": int64 [H, W]
    (the zone's label at every pixel, -1 outside the zones and in zones left without a label), "probs", "labels": what
    `classify_scene` returned}.  ``scene_confusion(result["map"], truth, K, cell=1)`` scores the map pixel by pixel."""
    from .scene import _host_plan, _classify
    plan = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, invalid_rule, windows, blend=blend,
                      border=border, fill=fill, anchor=anchor, mlp=mlp)
    if not blend and plan.stride != plan.patch:
        raise RuntimeError(f"blend=False needs stride == patch ({plan.patch}): overlapping windows give a pixel no single class without "
                           f"blending, got stride {plan.stride}")
    h, w = int(scene.shape[1]), int(scene.shape[2])
    if not isinstance(zones, torch.Tensor) or tuple(zones.shape) != (h, w):
        got = tuple(zones.shape) if isinstance(zones, torch.Tensor) else type(zones).__name__
        raise RuntimeError(f"zones must be a [H, W] = {[h, w]} zone raster of the scene's size, got {got}")
    _zones_arg(zones)
    if zones.device != scene.device:
        raise RuntimeError(f"zones is on {zones.device}, the scene on {scene.device}")
    k = int(mlp.num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise RuntimeError(f"the MLP's num_classes must be in 1..64, got {k}")
    rule = _rule_arg(rule)
    min_coverage = _coverage_arg(min_coverage)
    if num_zones is not None:
        num_zones = _num_zones_arg(num_zones, k)
    _require_gpu(scene.device)
    if num_zones is None:
        num_zones = _num_zones_arg(max(int(zones.max()) + 1, 1), k)             # the read-back; no zone at all: one empty zone
    probs, labels = _classify(plan, mlp, blend)
    zones = _native_zones(zones)
    stats = zonal_stats(zones, num_zones, labels, k, probs=probs, cell=plan.stride, origin=(plan.pads[0], plan.pads[2]))
    label, confidence, coverage = zone_labels(stats, rule, min_coverage)
    return {"zone_labels": label, "confidence": confidence, "coverage": coverage, "stats": stats,
            "map": paint_zones(zones, label, fill=-1), "probs": probs, "labels": labels}


# ---------------------------------------------------------------------------------------------------- zone_confusion
def zone_confusion(pred_labels, truth_labels, num_classes):
    """Object-level confusion counts int64 [K+1, K+1], one count per zone: counts[r, c] with r = the zone's truth label in [0, K),
    else K (no truth), and c = its predicted label in [0, K), else K (no label: -1) -- `scene_confusion`'s layout, so
    `report.confusion_metrics` reads it.  Truth per zone: ``zone_labels(zonal_stats(zones, Z, truth_raster, K), "votes")[0]``.
    Plain torch on Z entries (device or CPU)."""
    k = _int_arg(num_classes, "num_classes", 1, MAX_CLASSES)
    for name, t in (("pred_labels", pred_labels), ("truth_labels", truth_labels)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or not _is_int_tensor(t):
            raise RuntimeError(f"{name} must be a 1-D integer tensor, one label per zone")
    if pred_labels.shape != truth_labels.shape:
        raise RuntimeError(f"pred_labels has {pred_labels.numel()} zones, truth_labels {truth_labels.numel()}")
    if pred_labels.device != truth_labels.device:
        raise RuntimeError(f"pred_labels is on {pred_labels.device}, truth_labels on {truth_labels.device}")
    p, t = pred_labels.to(torch.int64), truth_labels.to(torch.int64)
    c = torch.where((p >= 0) & (p < k), p, k)
    r = torch.where((t >= 0) & (t < k), t, k)
    return torch.bincount(r * (k + 1) + c, minlength=(k + 1) ** 2).reshape(k + 1, k + 1)
