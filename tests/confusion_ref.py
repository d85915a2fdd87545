"""NumPy restatement of the confusion counts of a cell map against a label raster (include/eae.h, "accuracy assessment"): explicit
index arithmetic per pixel, then np.add.at.  The reference of tests/test_gpu_scene_confusion.py."""
import numpy as np


def confusion_ref(truth, pred, k, cell=1, origin=(0, 0), mask=None, ignore=()):
    """int64 [k+1, k+1]: counts[r, c] over the pixels with mask == 0.  truth [H,W] integers, pred [cH,cW] integers of cell x cell
    cells, pixel (y, x) in cell ((y + oy) // cell, (x + ox) // cell); r = truth in [0, k) and not in ignore, else k; c = the cell's
    value in [0, k) when the cell lies inside the map, else k."""
    truth = np.asarray(truth).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    h, w = truth.shape
    c_h, c_w = pred.shape
    oy, ox = origin
    cy = (np.arange(h, dtype=np.int64)[:, None] + oy) // cell + np.zeros((1, w), dtype=np.int64)
    cx = (np.arange(w, dtype=np.int64)[None, :] + ox) // cell + np.zeros((h, 1), dtype=np.int64)
    inside = (cy < c_h) & (cx < c_w)
    pv = pred[np.minimum(cy, c_h - 1), np.minimum(cx, c_w - 1)]
    c = np.where(inside & (pv >= 0) & (pv < k), pv, k)
    labelled = (truth >= 0) & (truth < k)
    for v in ignore:
        labelled &= truth != v
    r = np.where(labelled, truth, k)
    keep = np.ones((h, w), dtype=bool) if mask is None else np.asarray(mask) == 0
    cm = np.zeros((k + 1, k + 1), dtype=np.int64)
    np.add.at(cm, (r[keep], c[keep]), 1)
    return cm
