"""Cluster latents on the device: k-means over the rows `encode_scene` returns, the unsupervised classification of a scene without labels.

The two halves of a Lloyd iteration are kernels of the C library (include/eae.h, "latent clustering"):
`eae_kmeans_assign` (nearest centroid in exact fp32 on the f32-input MFMA, running argmin in registers: no N x K distance matrix) and
`eae_kmeans_update` (per-cluster means from a one-hot product with fixed-order partial sums: no float atomics, so the centroids are
bitwise the same from run to run).  Everything here takes fp32 latents z [N, L] (contiguous, on a HIP device), 1 <= L <= 256,
1 <= K <= 256, and labels are int64 with -1 for a row that holds a NaN or an Inf.

- `kmeans_predict` is one assign call: labels and squared distances against given centroids;
- `kmeans_init` is k-means++ seeding without a host synchronisation;
- `kmeans_fit` runs Lloyd's iterations; with ``tol=None`` it never reads anything back;
- `cluster_scene` encodes a scene's windows (`encode_scene`, with `classify_scene`'s window selection) and clusters them, or with
  ``centroids=`` applies the clusters of one scene to another; windows that are not run hold -1 in the map.
`report.cluster_class_table` and `report.name_clusters` turn a handful of `window_labels` into names for the clusters.
"""
from __future__ import annotations

import numbers
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check
from ._args import MAX_L, _alloc_workspace, _int_arg, _label_counts, _rows_arg          # noqa: F401  (importable from here as before)
from .engine import _ptr, _stream, _require_gpu

MAX_K = 256


class KMeansResult(NamedTuple):
    """centroids [K,L] float32; labels [N] int64 (-1: non-finite row) and dist [N] float32 (squared distance, NaN for such a row), both
    belonging to `centroids`; counts [K] int64 rows per cluster; inertia: 0-d float64 device tensor, nansum of dist; n_iter: the number
    of centroid updates applied."""
    centroids: torch.Tensor
    labels: torch.Tensor
    dist: torch.Tensor
    counts: torch.Tensor
    inertia: torch.Tensor
    n_iter: int


# ---------------------------------------------------------------------------------------------------- host-side validation
def _k_arg(k, n=None):
    k = _int_arg(k, "k", 1, MAX_K)
    if n is not None and k > n:
        raise RuntimeError(f"k = {k} is greater than the number of rows to cluster ({n})")
    return k


def _centroids_arg(centroids, width, device=None):
    """Centroids [K, L]: float32, K in 1..256, the latent width, and (when known) the data's device."""
    k, cwidth = _rows_arg(centroids, "centroids", "[K, L]", MAX_K)
    if cwidth != int(width):
        raise RuntimeError(f"centroids have width {cwidth}, the latents {width}")
    if device is not None and centroids.device != device:
        raise RuntimeError(f"centroids are on {centroids.device}, the latents on {device}")
    return k


def _fit_args(n, width, k, max_iter, tol, init, device=None):
    """Everything `kmeans_fit` can reject without a device: returns (k, init) with k taken from an init tensor."""
    if isinstance(init, torch.Tensor):
        k = _k_arg(_centroids_arg(init, width, device), n)
    elif init == "kmeans++":
        k = _k_arg(k, n)
    else:
        raise RuntimeError(f"init must be 'kmeans++' or a [K, L] tensor, got {init!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or int(max_iter) < 0:
        raise RuntimeError(f"max_iter must be a non-negative integer, got {max_iter!r}")
    if tol is not None and not 0.0 <= float(tol) < 1.0:
        raise RuntimeError(f"tol must be None or in [0, 1), got {tol!r}")
    return k, init


# ---------------------------------------------------------------------------------------------------- the two C calls
def _assign(z, centroids, labels, dist, changed=None, have_prev=False):
    n, width = z.shape
    check(_lib.load().eae_kmeans_assign(_stream(), _ptr(z), n, width, _ptr(centroids), centroids.shape[0], _ptr(labels), int(have_prev),
                                        _ptr(dist), _ptr(changed)))


def _workspace(z, k):
    return _alloc_workspace(_lib.load().eae_kmeans_workspace_bytes(z.shape[0], z.shape[1], k), z.device)


def _update(z, labels, centroids, counts, ws):
    n, width = z.shape
    check(_lib.load().eae_kmeans_update(_stream(), _ptr(z), n, width, _ptr(labels), centroids.shape[0], _ptr(centroids), _ptr(counts),
                                        _ptr(ws), ws.numel()))


def _predict(z, centroids):
    labels = torch.empty(z.shape[0], dtype=torch.int64, device=z.device)
    dist = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _assign(z, centroids, labels, dist)
    return labels, dist


# ---------------------------------------------------------------------------------------------------- public functions
def kmeans_predict(z, centroids):
    """(labels int64 [N], dist float32 [N]): the nearest centroid of every row and the squared distance to it, compared in fp32; the
    lowest index wins a tie; a row with a NaN or an Inf gets -1 and NaN."""
    _, width = _rows_arg(z, "z", "[N, L]")
    _centroids_arg(centroids, width, z.device)
    _require_gpu(z.device)
    return _predict(z.contiguous(), centroids.contiguous())


def _pick(w, u):
    """Index drawn with probability w / sum(w): the first i whose running sum exceeds u * total, u in [0, 1).  A row of weight 0 is
    never the first to exceed anything; the clamp only catches u * total rounding up to the total."""
    cs = torch.cumsum(w, 0)
    return torch.searchsorted(cs, (u * cs[-1]).reshape(1), right=True).clamp_(max=w.numel() - 1)


def kmeans_init(z, k, seed=0):
    """k-means++ seeding (Arthur & Vassilvitskii 2007): centroids [k, L], each bitwise a row of z.  The first is drawn uniformly from
    the finite rows, each later one with probability proportional to the squared distance to the nearest pick so far (one
    `kmeans_predict` against the new pick, then a running minimum).  The k uniform draws come from
    ``torch.rand(k, dtype=float64, generator=torch.Generator().manual_seed(seed))`` on the host, once; pick j is
    ``searchsorted(cumsum(w), u[j] * total)``.  Nothing is read back.  Rows with a NaN or an Inf have weight 0 and are never picked.

    With fewer than k distinct finite rows every remaining distance is 0: the draw then falls back to the uniform weights of the
    first pick and repeats a row.  A repeated centroid never wins a tie against its lower-indexed twin, so its cluster stays empty
    (and `kmeans_fit` leaves an empty cluster's centroid where it is)."""
    n, width = _rows_arg(z, "z", "[N, L]")
    k = _k_arg(k, n)
    _require_gpu(z.device)
    z = z.contiguous()
    u = torch.rand(k, dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed))).pin_memory().to(z.device, non_blocking=True)
    cent = torch.empty((k, width), dtype=torch.float32, device=z.device)
    finite = ~torch.isnan(_predict(z, torch.zeros((1, width), dtype=torch.float32, device=z.device))[1])
    w0 = finite.to(torch.float64)
    mind = None
    for j in range(k):
        if j == 0:
            w = w0
        else:
            w = torch.where(finite, mind, 0.0).to(torch.float64)
            w = torch.where(w.sum() > 0, w, w0)
        torch.index_select(z, 0, _pick(w, u[j]), out=cent[j:j + 1])
        if j + 1 < k:
            d = _predict(z, cent[j:j + 1])[1]
            mind = d if mind is None else torch.minimum(mind, d)
    return cent


def kmeans_fit(z, k, max_iter=100, tol=0.0, init="kmeans++", seed=0):
    """Lloyd's k-means over z [N, L]: `KMeansResult`.

    init: "kmeans++" (`kmeans_init` with `seed`) or a float32 [K, L] tensor of starting centroids (k is then taken from it).
    Each pass assigns every row to its nearest centroid, and from the second pass on counts the rows whose label changed; with
    ``tol`` a number the count is read back (8 bytes, the loop's one host readback) and the loop stops, before updating, when
    changed <= tol * N -- ``tol=0.0``: when no label changed, the fixed point.  Otherwise the centroids become the means of their rows
    (an empty cluster keeps its centroid) and the next pass begins.  ``tol=None`` runs exactly `max_iter` updates and reads nothing
    back.  When the loop ends by `max_iter`, one more assign makes the returned labels and distances belong to the returned centroids.
    The whole fit is bitwise repeatable: same data, same init, same result."""
    n, width = _rows_arg(z, "z", "[N, L]")
    k, init = _fit_args(n, width, k, max_iter, tol, init, z.device)
    _require_gpu(z.device)
    z = z.contiguous()
    dev = z.device
    cent = init.detach().clone().contiguous() if isinstance(init, torch.Tensor) else kmeans_init(z, k, seed)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    changed = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(z, k)
    n_iter, settled = 0, False
    with torch.cuda.device(dev):
        for it in range(int(max_iter)):
            _assign(z, cent, labels, dist, changed, have_prev=it > 0)
            if tol is not None and it > 0 and int(changed.item()) <= float(tol) * n:
                settled = True
                break
            _update(z, labels, cent, counts, ws)
            n_iter += 1
        if not settled:
            _assign(z, cent, labels, dist)
    return KMeansResult(cent, labels, dist, _label_counts(labels, k), dist.to(torch.float64).nansum(), n_iter)     # the RETURNED labels


def cluster_scene(scene, encoder, k=None, centroids=None, divisor=1.0, stride=None, batch=512, nodata=None, mask=None, max_invalid=0.0,
                  rule="all", windows=None, border=None, fill=0, anchor="center", max_iter=100, tol=0.0, seed=0):
    """(cluster_map int64 [nH, nW], `KMeansResult`): the unsupervised classification of a scene.  The windows are taken as
    `classify_scene` takes them -- the whole grid, the ids in ``windows=``, or under ``nodata=`` / ``mask=`` the valid windows
    (one host readback) -- encoded as `encode_scene` encodes them and clustered by `kmeans_fit(z, k, max_iter, tol, seed=seed)`;
    the result's rows are in the order of that window set.  Windows that are not run hold -1 in the map, as does a window whose
    latent row is not finite.

    centroids: a float32 [K, L] tensor (L = the encoder's latent_dim) switches to prediction only, the clusters of one scene applied
    to another: `kmeans_predict` against them, ``k`` is ignored, and the result carries those centroids with ``n_iter = 0``.

    Rejected before anything runs on the device: neither ``k`` nor ``centroids``; k outside 1..256 or greater than the number of
    windows to run (under nodata / mask that number is known only after the valid windows are counted: then it is checked right
    after, before the encoder runs); centroids of another width, dtype or device; and everything `classify_scene` rejects."""
    from .scene import _host_plan, _scene_latents
    h = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, allow_empty=False, border=border,
                   fill=fill, anchor=anchor)
    width = int(h.enc.latent_dim)
    if centroids is not None:
        _centroids_arg(centroids, width, scene.device)
    elif k is None:
        raise RuntimeError("cluster_scene needs k (to fit) or centroids (to predict)")
    else:
        _fit_args(h.n_max, width, k, max_iter, tol, "kmeans++")

    def admit(n):                                       # fewer valid windows than the host could know
        if n == 0 or (centroids is None and n < int(k)):
            raise RuntimeError(f"only {n} valid windows: nothing to cluster into k = {k}" if centroids is None else "no valid window")

    ids, z = _scene_latents(h, admit)
    if centroids is not None:
        cent = centroids.contiguous()
        labels, dist = _predict(z, cent)
        res = KMeansResult(cent, labels, dist, _label_counts(labels, cent.shape[0]), dist.to(torch.float64).nansum(), 0)
    else:
        res = kmeans_fit(z, int(k), max_iter=max_iter, tol=tol, seed=seed)
    return h.scatter(ids, res.labels, -1), res
