"""NumPy restatement of the zonal statistics (include/eae.h, "zonal statistics"): explicit index arithmetic per pixel, then np.add.at on
int64; the quantiser q; the per-zone decision of `zone_labels`; and the painting.  The reference of tests/test_gpu_zonal.py and
tests/test_zonal_reference.py."""
import numpy as np


def q_ref(p):
    """q(p) = rint(2^32 * min(max(p, 0), 1)) in float64, round-half-even, q(NaN) = 0."""
    return np.rint(np.clip(np.nan_to_num(np.asarray(p).astype(np.float64), nan=0.0), 0, 1) * 2 ** 32).astype(np.int64)


def zonal_ref(zones, z_count, labels, k, probs=None, cell=1, origin=(0, 0), mask=None):
    """(votes int64 [Z, k+1], prob_sums int64 [Z, k] or None) over the pixels with mask == 0 whose zone id is in [0, Z).  labels
    [cH, cW] integers of cell x cell cells, pixel (y, x) in cell ((y + oy) // cell, (x + ox) // cell); c = the cell's label in [0, k)
    when the cell lies inside the map, else k; with probs [k, cH, cW] and c < k every class j receives q(probs[j, cell])."""
    zones = np.asarray(zones).astype(np.int64)
    labels = np.asarray(labels).astype(np.int64)
    h, w = zones.shape
    c_h, c_w = labels.shape
    oy, ox = origin
    cy = (np.arange(h, dtype=np.int64)[:, None] + oy) // cell + np.zeros((1, w), dtype=np.int64)
    cx = (np.arange(w, dtype=np.int64)[None, :] + ox) // cell + np.zeros((h, 1), dtype=np.int64)
    inside = (cy < c_h) & (cx < c_w)
    cyc, cxc = np.minimum(cy, c_h - 1), np.minimum(cx, c_w - 1)
    lv = labels[cyc, cxc]
    c = np.where(inside & (lv >= 0) & (lv < k), lv, k)
    keep = (zones >= 0) & (zones < z_count)
    if mask is not None:
        keep &= np.asarray(mask) == 0
    votes = np.zeros((z_count, k + 1), dtype=np.int64)
    np.add.at(votes, (zones[keep], c[keep]), 1)
    if probs is None:
        return votes, None
    q = q_ref(probs)                                          # [k, cH, cW]
    sums = np.zeros((z_count, k), dtype=np.int64)
    voted = keep & (c < k)
    zz, yy, xx = zones[voted], cyc[voted], cxc[voted]
    for j in range(k):
        np.add.at(sums[:, j], zz, q[j, yy, xx])
    return votes, sums


def zone_labels_ref(votes, prob_sums, rule="probs", min_coverage=0.0):
    """(label int64 [Z], confidence float32 [Z], coverage float32 [Z]), zone by zone in Python integers: the lowest class among the
    maxima; no label where classified == 0 or float(classified) < min_coverage * float(total)."""
    votes = np.asarray(votes)
    z_count, k = votes.shape[0], votes.shape[1] - 1
    label = np.full(z_count, -1, dtype=np.int64)
    conf = np.full(z_count, np.nan, dtype=np.float32)
    cov = np.full(z_count, np.nan, dtype=np.float32)
    for z in range(z_count):
        row = [int(v) for v in votes[z]]
        total, classified = sum(row), sum(row[:k])
        if total:
            cov[z] = np.float32(np.float64(classified) / np.float64(total))
        if classified == 0 or np.float64(classified) < np.float64(min_coverage) * np.float64(total):
            continue
        table = [int(v) for v in prob_sums[z]] if rule == "probs" else row[:k]
        best = max(table)
        label[z] = table.index(best)
        denom = np.float64(classified) * (2.0 ** 32 if rule == "probs" else 1.0)
        conf[z] = np.float32(np.float64(best) / denom)
    return label, conf, cov


def paint_ref(zones, values, fill=-1):
    """int64 [H, W]: values[zones] where the id is in [0, len(values)), else fill."""
    zones = np.asarray(zones).astype(np.int64)
    values = np.asarray(values).astype(np.int64)
    ok = (zones >= 0) & (zones < values.shape[0])
    return np.where(ok, values[np.where(ok, zones, 0)], fill).astype(np.int64)


def compact_ref(ids):
    """(zones int32 [H, W], ids int64 [Z]): the distinct non-negative values numbered in ascending order, negatives -> -1."""
    ids = np.asarray(ids).astype(np.int64)
    values = sorted(set(int(v) for v in ids.ravel() if v >= 0))
    index = {v: i for i, v in enumerate(values)}
    zones = np.array([[index.get(int(v), -1) for v in row] for row in ids], dtype=np.int32).reshape(ids.shape)
    return zones, np.array(values, dtype=np.int64)
