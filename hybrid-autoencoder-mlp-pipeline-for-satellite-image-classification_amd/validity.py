"""How good is a clustering or a labelling of the latent space: silhouettes, a table of class separation, and the choice of k.

One entry point of the C library does the pairwise work (include/eae.h, "latent validity"):
`eae_class_dist_sums` adds, for every query row, its Euclidean distances to the bank rows of each class, scored in exact fp32 on the
f32-input MFMA as `eae_knn_search` scores neighbours.  No N x N distance matrix is made, nothing is read back, there are no float
atomics and every result is bitwise repeatable.  Everything here takes fp32 latents [rows, L] on a HIP device, 1 <= L <= 256, and
int64 labels in -1..K-1, 1 <= K <= 256; a row that is labelled -1 or out of range, or that holds a NaN or an Inf, belongs to no class.

- `class_distance_sums` is the kernel call: sums [Nq, K] of distances by class, and the class sizes;
- `silhouette_samples` / `silhouette_score` are scikit-learn's silhouette coefficient (Euclidean by default), per row, per class and
  overall, optionally from a sample of the rows against the whole set;
- `class_distance_matrix` is the K x K table of mean distances between classes (`report.separation_table` prints it);
- `davies_bouldin_score` and `calinski_harabasz_score` are the two cheap indices, float64 torch ops;
- `select_k` runs `kmeans_fit` over several k and picks one by a criterion.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check
from ._args import _alloc_workspace, _int_arg, _label_counts, _rows_arg
from .cluster import MAX_K, _fit_args, _update, _workspace, kmeans_fit
from .engine import _ptr, _stream, _require_gpu

METRICS = ("euclidean", "sqeuclidean")
CRITERIA = ("silhouette", "calinski_harabasz", "davies_bouldin")


# ---------------------------------------------------------------------------------------------------- host-side validation
def _labels_arg(labels, rows, name="labels", device=None):
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype != torch.int64:
        raise RuntimeError(f"{name} must be a 1-D int64 tensor, one label per row")
    if int(labels.numel()) != int(rows):
        raise RuntimeError(f"{name} has {labels.numel()} entries for {rows} rows")
    if device is not None and labels.device != device:
        raise RuntimeError(f"{name} are on {labels.device}, the rows on {device}")


def _metric_arg(metric):
    if metric not in METRICS:
        raise RuntimeError(f"metric must be one of {METRICS}, got {metric!r}")
    return METRICS.index(metric)


def _sums_args(q, bank, labels, num_classes, metric, self_index):
    nq, width = _rows_arg(q, "q", "[Nq, L]")
    m, bwidth = _rows_arg(bank, "bank", "[M, L]")
    if width != bwidth:
        raise RuntimeError(f"q has width {width}, the bank {bwidth}")
    if q.device != bank.device:
        raise RuntimeError(f"q is on {q.device}, the bank on {bank.device}")
    _labels_arg(labels, m, "labels", bank.device)
    k = _int_arg(num_classes, "num_classes", 1, MAX_K)
    if self_index is not None:
        _labels_arg(self_index, nq, "self_index", bank.device)
    return nq, m, width, k, _metric_arg(metric)


def _z_args(z, labels, num_classes, allow_none=False):
    n, width = _rows_arg(z, "z", "[N, L]")
    _labels_arg(labels, n, "labels", z.device)
    if num_classes is None and allow_none:
        return n, width, None
    return n, width, _int_arg(num_classes, "num_classes", 1, MAX_K)


def _sample_arg(sample, n):
    return None if sample is None else _int_arg(sample, "sample", 1, n)


def _num_classes(labels, num_classes):
    """K given, or (the one readback of this module's metrics) the greatest label + 1."""
    if num_classes is not None:
        return num_classes
    return _int_arg(max(int(labels.max().item()) + 1, 1), "num_classes (labels.max() + 1)", 1, MAX_K)


def _sample_rows(n, sample, seed, device):
    """The query rows of ``sample=``: ``torch.randperm(N, generator=manual_seed(seed))[:sample]`` drawn on the host; None for all."""
    if sample is None:
        return None
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:sample].to(device)


# ---------------------------------------------------------------------------------------------------- the C call
def _clean(bank, labels, k):
    """Labels with -1 for every row that joins no class: labelled outside [0, k), or not finite.  A row is taken as finite when the sum of
    its values is (a NaN or an Inf anywhere makes the sum NaN or Inf; so do finite values whose sum overflows, and their squared norm
    would): one float a row instead of an [M, L] temporary."""
    ok = torch.isfinite(bank.sum(dim=1)) & (labels >= 0) & (labels < k)
    return torch.where(ok, labels, -1)


def _sums(q, bank, lab, k, metric, self_index, center):
    """`eae_class_dist_sums` on contiguous fp32 device tensors and cleaned labels: (sums, counts)."""
    nq, width = q.shape
    m = bank.shape[0]
    dev = bank.device
    counts = _label_counts(lab, k)
    order = torch.sort(lab, stable=True).indices                           # the rows of no class first, then class by class
    seg = torch.cat([(m - counts.sum()).reshape(1), counts]).cumsum(0)     # [K+1]: seg[0] = the number of unclassed rows
    sbank = bank.index_select(0, order)                                    # the one copy of the bank; what follows is in place
    if center:
        sbank.masked_fill_((lab.index_select(0, order) < 0)[:, None], 0.0)     # rows of no class: the kernel never reads them
        mu = sbank.sum(0) / counts.sum().clamp(min=1)                      # fp32 throughout: any vector near the mean serves
        sbank.sub_(mu)
        q = q - mu
    self_pos = None
    if self_index is not None:
        inv = torch.empty(m, dtype=torch.int64, device=dev)
        inv[order] = torch.arange(m, dtype=torch.int64, device=dev)
        inside = (self_index >= 0) & (self_index < m)
        self_pos = torch.where(inside, inv[self_index.clamp(0, m - 1)], -1)
    lib = _lib.load()
    nbytes = lib.eae_class_dist_workspace_bytes(nq, m, width, k)
    ws = _alloc_workspace(nbytes, dev, or_none=True)
    sums = torch.empty((nq, k), dtype=torch.float32, device=dev)
    q = q.contiguous()
    with torch.cuda.device(dev):
        check(lib.eae_class_dist_sums(_stream(), _ptr(q), nq, _ptr(sbank), m, width, _ptr(seg), k, _ptr(self_pos), metric, _ptr(sums),
                                      _ptr(ws), nbytes))
    return sums, counts


def class_distance_sums(q, bank, labels, num_classes, metric="euclidean", self_index=None, center=True):
    """(sums float32 [Nq, K], counts int64 [K]): sums[n, c] is the sum of the distances from q[n] to the bank rows of class c, counts
    the rows per class.  labels: int64 [M] in -1..K-1; bank rows labelled -1 or out of range, or holding a NaN or an Inf, join no
    class.  A query row with a NaN or an Inf gets a row of NaN; an empty class gives 0.

    metric: "euclidean" or "sqeuclidean".  self_index: int64 [Nq], the bank row that is query n itself and is left out of its sums
    (-1: none).  center: subtract the fp32 mean of the classed bank rows from both sides first -- distances are translation
    invariant, and the fp32 error of a pair's squared distance grows with (||q|| + ||b||)^2.

    The bank is sorted by class (a stable `torch.sort` of the cleaned labels, one gather) and handed to `eae_class_dist_sums` with
    the segment starts; self_index goes through the inverse permutation.  Nothing is read back."""
    _, _, _, k, metric = _sums_args(q, bank, labels, num_classes, metric, self_index)
    _require_gpu(bank.device)
    bank = bank.contiguous()
    return _sums(q if q is bank else q.contiguous(), bank, _clean(bank, labels, k), k, metric, self_index, center)


# ---------------------------------------------------------------------------------------------------- silhouettes
def _silhouette(z, labels, k, metric, rows):
    """(s float64 [Nq], lab int64 [Nq]) of the query rows `rows` (None: all) against all of z: the silhouette and the cleaned label."""
    z = z.contiguous()
    lab = _clean(z, labels, k)
    if rows is None:
        q, qlab, self_index = z, lab, torch.arange(z.shape[0], dtype=torch.int64, device=z.device)
    else:
        q, qlab, self_index = z.index_select(0, rows), lab[rows], rows
    sums, counts = _sums(q, z, lab, k, metric, self_index, True)
    own = qlab.clamp(min=0)[:, None]
    n_own = counts[qlab.clamp(min=0)]
    a = sums.gather(1, own).squeeze(1).to(torch.float64) / (n_own - 1).clamp(min=1)
    other = sums.to(torch.float64)                                         # the one float64 [Nq, K] array; what follows is in place
    del sums
    other.div_(counts.clamp(min=1)[None, :]).masked_fill_((counts == 0)[None, :], float("inf")).scatter_(1, own, float("inf"))
    b = other.min(dim=1).values
    top = torch.maximum(a, b)
    s = torch.where(top > 0, (b - a) / top, 0.0)
    s = torch.where(n_own > 1, s, 0.0)                                     # a class of one row: 0, scikit-learn's convention
    nan = torch.full_like(s, float("nan"))
    s = torch.where((qlab >= 0) & ((counts > 0).sum() >= 2), s, nan)
    return s, qlab


def silhouette_samples(z, labels, num_classes=None, metric="euclidean"):
    """float32 [N]: the silhouette coefficient s = (b - a) / max(a, b) of every row, a the mean distance to the other rows of its own
    class, b the least mean distance to the rows of another non-empty class; scikit-learn's `silhouette_samples`.  A class of one row
    gives 0, as does max(a, b) = 0; a row labelled -1 (or out of range) or holding a NaN or an Inf gives NaN; fewer than two non-empty
    classes give NaN everywhere (the counts stay on the device, so this cannot raise).  From the sums on, float64 torch ops.
    ``num_classes=None`` reads ``labels.max()`` back, the one case that synchronises."""
    _, _, k = _z_args(z, labels, num_classes, allow_none=True)
    _metric_arg(metric)
    _require_gpu(z.device)
    k = _num_classes(labels, k)
    return _silhouette(z, labels, k, METRICS.index(metric), None)[0].to(torch.float32)


def _segment_sums(values, lab, k):
    """float64 [K, ...]: the sums of `values` (float64 [N, ...]) over the rows of each label in [0, k), by a stable sort and the
    differences of one running sum at the segment ends -- no atomics, so the same bits every run.  Rows of label -1 are skipped."""
    counts = _label_counts(lab, k)
    order = torch.sort(lab, stable=True).indices
    run = torch.cumsum(values.index_select(0, order), 0)
    run = torch.cat([torch.zeros_like(run[:1]), run])
    seg = torch.cat([(lab.numel() - counts.sum()).reshape(1), counts]).cumsum(0)
    return run.index_select(0, seg[1:]) - run.index_select(0, seg[:-1]), counts


def silhouette_score(z, labels, num_classes=None, metric="euclidean", sample=None, seed=0):
    """(score, per_class): the mean silhouette over the rows that have one (a 0-d float64 device tensor, the nanmean) and the mean per
    class (float64 [K], NaN for a class without such a row).  sample=n takes the silhouettes of n rows only, drawn without
    replacement as ``torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:n]`` on the host, each against ALL rows: n N
    pairs instead of N^2."""
    n, _, k = _z_args(z, labels, num_classes, allow_none=True)
    _metric_arg(metric)
    sample = _sample_arg(sample, n)
    _require_gpu(z.device)
    k = _num_classes(labels, k)
    s, qlab = _silhouette(z, labels, k, METRICS.index(metric), _sample_rows(n, sample, seed, z.device))
    has = ~torch.isnan(s)
    lab = torch.where(has, qlab, -1)
    tot, cnt = _segment_sums(torch.where(has, s, 0.0), lab, k)
    return s.nanmean(), torch.where(cnt > 0, tot / cnt.clamp(min=1), float("nan"))


def class_distance_matrix(z, labels, num_classes, sample=None, seed=0):
    """float32 [K, K]: entry (a, b) is the mean Euclidean distance from the rows of class a to the rows of class b; the diagonal is
    over distinct pairs (NaN for a class of one row).  Rows and columns of empty classes are NaN.  sample=n averages over n query rows
    (drawn as `silhouette_score` draws them) against all rows; a class without a sampled row has a NaN row.

    It is the mean, by query class, of the rows of sums / counts: `eae_kmeans_update`'s fixed-order one-hot product, taking width K
    as it takes L.  So the table is bitwise repeatable.  The diagonal is rescaled by n_a / (n_a - 1)."""
    n, _, k = _z_args(z, labels, num_classes)
    sample = _sample_arg(sample, n)
    _require_gpu(z.device)
    z = z.contiguous()
    lab = _clean(z, labels, k)
    rows = _sample_rows(n, sample, seed, z.device)
    if rows is None:
        q, qlab, self_index = z, lab, torch.arange(n, dtype=torch.int64, device=z.device)
    else:
        q, qlab, self_index = z.index_select(0, rows), lab[rows], rows
    sums, counts = _sums(q, z, lab, k, 0, self_index, True)
    filled = counts > 0
    mean = torch.where(filled[None, :], sums / counts.clamp(min=1)[None, :].to(torch.float32), 0.0)
    mean = torch.where((qlab >= 0)[:, None], mean, 0.0).contiguous()       # rows of no class carry NaN and label -1: skipped, values and all
    out = torch.full((k, k), float("nan"), dtype=torch.float32, device=z.device)
    seen = torch.empty(k, dtype=torch.int64, device=z.device)
    with torch.cuda.device(z.device):
        _update(mean, qlab.contiguous(), out, seen, _workspace(mean, k))
    nf = counts.to(torch.float32)
    scale = torch.where(counts > 1, nf / (nf - 1).clamp(min=1), float("nan"))
    out = torch.where(torch.eye(k, dtype=torch.bool, device=z.device), out * scale[:, None], out)
    return torch.where(filled[None, :] & (seen > 0)[:, None], out, float("nan"))


# ---------------------------------------------------------------------------------------------------- the two cheap indices
def _class_stats(z, labels, k):
    """float64: (centroids [K, L], counts [K], sq [N] squared distance of every classed row to its centroid -- 0 for the others, lab)."""
    lab = _clean(z, labels, k)
    z64 = torch.where((lab >= 0)[:, None], z.to(torch.float64), 0.0)
    tot, counts = _segment_sums(z64, lab, k)
    cent = tot / counts.clamp(min=1)[:, None]
    diff = torch.where((lab >= 0)[:, None], z64 - cent.index_select(0, lab.clamp(min=0)), 0.0)
    return cent, counts, (diff * diff).sum(1), lab


def davies_bouldin_score(z, labels, num_classes):
    """0-d float64 device tensor: scikit-learn's `davies_bouldin_score` over the non-empty classes -- the mean over classes i of
    max_{j != i} (s_i + s_j) / ||c_i - c_j||, s the mean distance of a class's rows to its centroid c; lower is better.  Two equal
    centroids contribute nothing (scikit-learn's convention).  NaN with fewer than two non-empty classes.  float64 torch ops; the class
    sums are segment sums after a stable sort, not `index_add_`."""
    _, _, k = _z_args(z, labels, num_classes)
    _require_gpu(z.device)
    return _davies_bouldin(z.contiguous(), labels, k)


def _davies_bouldin(z, labels, k):
    cent, counts, sq, lab = _class_stats(z, labels, k)
    spread = _segment_sums(sq.sqrt(), lab, k)[0] / counts.clamp(min=1)
    gap = torch.cdist(cent, cent, compute_mode="donot_use_mm_for_euclid_dist")
    filled = counts > 0
    pair = filled[:, None] & filled[None, :] & (gap > 0)
    ratio = torch.where(pair, (spread[:, None] + spread[None, :]) / torch.where(pair, gap, 1.0), 0.0)
    worst = torch.where(filled, ratio.max(dim=1).values, 0.0)
    nk = filled.sum()
    return torch.where(nk >= 2, worst.sum() / nk.clamp(min=1), float("nan"))


def calinski_harabasz_score(z, labels, num_classes):
    """0-d float64 device tensor: scikit-learn's `calinski_harabasz_score` over the classed rows and the k non-empty classes --
    (between-class dispersion / (k - 1)) / (within-class dispersion / (n - k)); higher is better; 1 when the within-class dispersion
    is 0, NaN with fewer than two non-empty classes.  float64 torch ops on segment sums."""
    _, _, k = _z_args(z, labels, num_classes)
    _require_gpu(z.device)
    return _calinski_harabasz(z.contiguous(), labels, k)


def _calinski_harabasz(z, labels, k):
    cent, counts, sq, _ = _class_stats(z, labels, k)
    n = counts.sum()
    nk = (counts > 0).sum()
    cf = counts.to(torch.float64)
    mean = (cent * cf[:, None]).sum(0) / n.clamp(min=1)
    between = (cf * ((cent - mean) ** 2).sum(1)).sum()
    within = sq.sum()
    score = torch.where(within > 0, between * (n - nk) / (within * (nk - 1).clamp(min=1)), 1.0)
    return torch.where(nk >= 2, score, float("nan"))


# ---------------------------------------------------------------------------------------------------- the choice of k
def _select_args(z, ks, criterion, sample, max_iter, tol):
    n, width = _rows_arg(z, "z", "[N, L]")
    if criterion not in CRITERIA:
        raise RuntimeError(f"criterion must be one of {CRITERIA}, got {criterion!r}")
    try:
        ks = list(ks)
    except TypeError:
        raise RuntimeError(f"ks must be a sequence of integers, got {ks!r}") from None
    if not ks:
        raise RuntimeError("ks is empty")
    for k in ks:
        _fit_args(n, width, k, max_iter, tol, "kmeans++")                  # k in 1..256 and k <= N, max_iter, tol
    return n, [int(k) for k in ks], _sample_arg(sample, n)


def select_k(z, ks, criterion="silhouette", sample=None, max_iter=100, tol=0.0, seed=0):
    """(best_k, scores {k: float}, results {k: `KMeansResult`}): `kmeans_fit(z, k, max_iter, tol, seed=seed)` for every k in ks, each
    scored by ``criterion``: "silhouette" (`silhouette_score`, over ``sample=`` rows when given) and "calinski_harabasz" are
    maximised, "davies_bouldin" is minimised.  The score of every k is read back (one readback per k beyond the fit's own); a k whose
    score is NaN (k = 1, or a fit that left one cluster) is never chosen unless every score is NaN; ties go to the smaller k."""
    n, ks, sample = _select_args(z, ks, criterion, sample, max_iter, tol)
    _require_gpu(z.device)
    z = z.contiguous()
    scores, results = {}, {}
    for k in ks:
        res = kmeans_fit(z, k, max_iter=max_iter, tol=tol, seed=seed)
        if criterion == "silhouette":
            score = _silhouette(z, res.labels, k, 0, _sample_rows(n, sample, seed, z.device))[0].nanmean()
        elif criterion == "calinski_harabasz":
            score = _calinski_harabasz(z, res.labels, k)
        else:
            score = _davies_bouldin(z, res.labels, k)
        scores[k], results[k] = float(score.item()), res
    sign = 1.0 if criterion == "davies_bouldin" else -1.0
    best = min(scores, key=lambda k: (scores[k] != scores[k], sign * scores[k] if scores[k] == scores[k] else 0.0, k))
    return best, scores, results
