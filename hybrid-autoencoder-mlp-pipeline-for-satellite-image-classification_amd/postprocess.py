"""Clean class maps on the device: majority filter, connected regions, their table, and a sieve.

The maps `classify_scene`, `cluster_scene` and `knn_classify_scene` return are speckled at the level of windows and cells; these
functions smooth them before `scene_confusion` scores them, without a trip to the host.  The kernels are those of the C library
(include/eae.h, "map post-processing").

A map is an int64 [H, W] tensor on a HIP device, as `classify_scene` returns it: values in [0, num_classes) are classes,
num_classes in 1..64 (`scene_confusion`'s limit), every other value -- the -1 of a window that was not run included -- is
"unclassified".  H, W >= 1 and H * W < 2^31.  Every function is stateless, runs on the current stream and reads nothing back unless
it says so; all results are integers that the semantics define uniquely, so they are identical from run to run.  `label_regions`,
`region_table` and `sieve` also take ``num_classes=None``: the map then holds arbitrary labels (cluster ids, parcel ids), any value
>= 0 a label compared on all 64 bits, negatives unclassified (`eae_map_regions_wide`; `segment.py` builds its zones this way).

- `majority_filter`: the mode of the classified cells of a clipped (2r+1)^2 window, `passes` times;
- `label_regions`: connected regions (4- or 8-connectivity), a region's id the smallest linear index y * W + x of its cells;
- `region_table`: id, class, area and bounding box of every region (one host read-back, for the number of regions);
- `sieve`: regions smaller than `min_size` cells dissolve into their largest edge neighbour that is not small (what `gdal_sieve` does).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check
from ._args import _alloc_workspace, _int_arg
from .engine import _ptr, _stream, _require_gpu

MAX_CLASSES = 64
MAX_RADIUS = 7
_CELL_LIMIT = 2 ** 31


# ---------------------------------------------------------------------------------------------------- host-side validation
def _map_arg(t, what="labels"):
    """(H, W) of an int64 [H, W] map with H, W >= 1 and H * W < 2^31."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.int64:
        got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} must be a 2-D int64 map [H, W], got {got}")
    h, w = int(t.shape[0]), int(t.shape[1])
    if h < 1 or w < 1:
        raise RuntimeError(f"{what} is empty: {[h, w]}")
    if h * w >= _CELL_LIMIT:
        raise RuntimeError(f"{what} has {h} x {w} cells: H * W must be below 2^31")
    return h, w


def _classes_arg(k, wide=False):
    """num_classes in 1..64; with ``wide``, None as well: any non-negative value of the map is then a label."""
    if wide and k is None:
        return None
    return _int_arg(k, "num_classes", 1, MAX_CLASSES)


def _device_arg(device, k):
    """`_require_gpu`, naming the path the caller asked for when that is the one over arbitrary labels."""
    if k is None and (device.type != "cuda" or not torch.cuda.is_available()):
        raise RuntimeError("num_classes=None (arbitrary labels) runs on a HIP device only, like every function here; there is no CPU path")
    _require_gpu(device)


def _connectivity_arg(c):
    if isinstance(c, bool) or c not in (4, 8):
        raise RuntimeError(f"connectivity must be 4 or 8, got {c!r}")
    return int(c)


def _workspace(h, w, device):
    return _alloc_workspace(_lib.load().eae_map_workspace_bytes(h, w), device)


# ---------------------------------------------------------------------------------------------------- the C calls
def _regions(labels, k, connectivity, ws):
    """k = None: `eae_map_regions_wide`, every value >= 0 a label."""
    h, w = labels.shape
    regions = torch.empty_like(labels)
    lib = _lib.load()
    if k is None:
        check(lib.eae_map_regions_wide(_stream(), _ptr(labels), h, w, connectivity, _ptr(regions), _ptr(ws), ws.numel()))
    else:
        check(lib.eae_map_regions(_stream(), _ptr(labels), h, w, k, connectivity, _ptr(regions), _ptr(ws), ws.numel()))
    return regions


def _stats(regions, with_bbox):
    h, w = regions.shape
    area = torch.empty(h * w, dtype=torch.int32, device=regions.device)
    bbox = torch.empty((h * w, 4), dtype=torch.int32, device=regions.device) if with_bbox else None
    check(_lib.load().eae_map_region_stats(_stream(), _ptr(regions), h, w, _ptr(area), _ptr(bbox)))
    return area, bbox


# ---------------------------------------------------------------------------------------------------- public functions
def majority_filter(labels, num_classes, radius=1, fill=False, passes=1):
    """int64 [H, W]: cell (y, x) becomes the most frequent class among the classified cells of the (2 radius + 1)^2 window centred on
    it, the window clipped at the map's edge; radius in 1..7.

    Ties: the centre's own class wins when it is among the tied classes, otherwise the lowest class id.  An unclassified centre stays
    as stored, unless ``fill=True`` and the window holds at least one classified cell: then it takes the winner.  ``passes`` >= 1:
    pass i reads the whole output of pass i - 1 (two buffers)."""
    h, w = _map_arg(labels)
    k = _classes_arg(num_classes)
    radius = _int_arg(radius, "radius", 1, MAX_RADIUS)
    passes = _int_arg(passes, "passes", 1, 2 ** 31 - 1)
    _require_gpu(labels.device)
    src = labels.contiguous()
    lib = _lib.load()
    bufs = [torch.empty_like(src), torch.empty_like(src) if passes > 1 else None]
    with torch.cuda.device(src.device):
        for i in range(passes):
            dst = bufs[i & 1]
            check(lib.eae_map_majority(_stream(), _ptr(src), h, w, k, radius, int(bool(fill)), _ptr(dst)))
            src = dst
    return src


def label_regions(labels, num_classes, connectivity=4):
    """regions int64 [H, W]: the region of every classified cell, -1 for an unclassified one.  A region is a maximal set of cells that
    share one class and are connected through edges (``connectivity=4``) or edges and corners (8).  A region's id is the smallest
    linear index y * W + x of its cells: the result is unique, whatever the launch geometry or the order in which tiles are merged.
    ``num_classes=None``: any non-negative value is a label, compared on all 64 bits (cluster ids, parcel ids), negatives are
    unclassified."""
    h, w = _map_arg(labels)
    k = _classes_arg(num_classes, wide=True)
    connectivity = _connectivity_arg(connectivity)
    _device_arg(labels.device, k)
    labels = labels.contiguous()
    with torch.cuda.device(labels.device):
        return _regions(labels, k, connectivity, _workspace(h, w, labels.device))


def region_table(labels, regions, num_classes=None):
    """The regions of `label_regions(labels, ...)` as a dict of device tensors, rows by ascending region id: ``id`` int64 [R], ``cls``
    int64 [R] (the class of the region's cells), ``area`` int64 [R] (cells) and ``bbox`` int64 [R, 4] = (y0, x0, y1, x1), inclusive.
    Areas and boxes are integer atomics on the device (exact); compacting them to R rows reads R back, the function's one host
    read-back.  The table is read off ``regions`` alone, so it is the same for class maps and for maps of arbitrary labels;
    ``num_classes`` (None, or what `label_regions` was given) is checked and otherwise unused."""
    h, w = _map_arg(labels)
    _classes_arg(num_classes, wide=True)
    if _map_arg(regions, "regions") != (h, w):
        raise RuntimeError(f"regions has shape {list(regions.shape)}, labels {[h, w]}")
    if regions.device != labels.device:
        raise RuntimeError(f"regions is on {regions.device}, labels on {labels.device}")
    _require_gpu(labels.device)
    labels, regions = labels.contiguous(), regions.contiguous()
    with torch.cuda.device(labels.device):
        area, bbox = _stats(regions, True)
    ids = torch.nonzero(area, as_tuple=False).reshape(-1)              # ascending; the read-back for R
    return {"id": ids, "cls": labels.reshape(-1)[ids], "area": area[ids].to(torch.int64), "bbox": bbox[ids].to(torch.int64)}


def sieve(labels, num_classes, min_size, connectivity=4, passes=1, return_changed=False):
    """int64 [H, W]: the map with its small regions dissolved.  One pass is decided entirely from that pass's input:

    1. regions and areas under ``connectivity`` (`label_regions`);
    2. a region is small when area < ``min_size`` (>= 1; 1 is the identity);
    3. the candidates of a small region are the regions that are not small and share a cell edge with it -- edges for both
       connectivities, as in GDAL: a diagonal touch is no neighbour;
    4. it takes the class of the candidate with the largest area, the lowest region id on a tie;
    5. a small region without a candidate (surrounded by unclassified cells or by small regions, or covering the map) stays;
    6. unclassified cells never change and are never candidates.

    Exactly ``passes`` passes run, each on the previous one's output, and nothing is read back.  ``return_changed=True``: returns
    (map, changed), changed a 0-d int64 device tensor, the number of cells whose class changed in the last pass.
    ``num_classes=None``: any non-negative value is a label (`label_regions`)."""
    h, w = _map_arg(labels)
    k = _classes_arg(num_classes, wide=True)
    min_size = _int_arg(min_size, "min_size", 1, 2 ** 63 - 1)
    connectivity = _connectivity_arg(connectivity)
    passes = _int_arg(passes, "passes", 1, 2 ** 31 - 1)
    _device_arg(labels.device, k)
    src = labels.contiguous()
    lib = _lib.load()
    changed = torch.empty((), dtype=torch.int64, device=src.device) if return_changed else None
    bufs = [torch.empty_like(src), torch.empty_like(src) if passes > 1 else None]
    with torch.cuda.device(src.device):
        ws = _workspace(h, w, src.device)
        for i in range(passes):
            regions = _regions(src, k, connectivity, ws)
            area, _ = _stats(regions, False)
            dst = bufs[i & 1]
            check(lib.eae_map_sieve_pass(_stream(), _ptr(src), _ptr(regions), _ptr(area), h, w, min_size, _ptr(dst), _ptr(changed),
                                         _ptr(ws), ws.numel()))
            src = dst
    return (src, changed) if return_changed else src
