"""Nearest neighbours over latents on the device: retrieval and kNN classification on the rows `encode_scene` returns.

One entry point of the C library does the search (include/eae.h, "latent neighbours"): `eae_knn_search` scores
every (query, bank row) pair in exact fp32 on the f32-input MFMA, streams the bank through the kernel and keeps each query's k best
in a sorted list on chip: no Nq x M distance matrix is written, equal scores are ordered by ascending bank index, and the result is
bitwise repeatable and independent of the launch geometry.  Everything here takes fp32 tensors [rows, L] on a HIP device,
1 <= L <= 256, 1 <= k <= 32; an index of -1 (with distance NaN) marks a slot with no neighbour: a query row that holds a NaN or an
Inf, or fewer than k eligible bank rows.  Bank rows that hold a NaN or an Inf are never returned.

- `knn_search` is the search itself: indices and squared L2 (or cosine) distances;
- `knn_classify` votes over the neighbours' labels (torch ops on the search result), uniformly or weighted by 1 / distance;
- `similar_windows` is query by example on a scene: the windows whose latents are nearest to given windows or latents;
- `knn_classify_scene` is the class map of a scene from a labelled bank of latents, without a trained classifier.
"""
from __future__ import annotations

import numbers
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check
from ._args import MAX_L, _int_arg, _alloc_workspace, _rows_arg       # noqa: F401  one width limit, one check of fp32 rows and of k
from .engine import _ptr, _stream, _require_gpu
from .scene import _host_plan, _scene_latents

MAX_K = 32
METRICS = ("l2", "cosine")


class KNNResult(NamedTuple):
    """idx [Nq,k] int64: bank rows by ascending (distance, index), -1 in an empty slot; dist [Nq,k] float32: squared L2 distance, or
    1 - cos under ``metric="cosine"``, NaN in an empty slot."""
    idx: torch.Tensor
    dist: torch.Tensor


# ---------------------------------------------------------------------------------------------------- host-side validation
def _search_args(queries, bank, k, exclude_self, metric, most=MAX_K):
    nq, width = _rows_arg(queries, "queries")
    m, bwidth = _rows_arg(bank, "bank")
    if width != bwidth:
        raise RuntimeError(f"queries have width {width}, the bank {bwidth}")
    if queries.device != bank.device:
        raise RuntimeError(f"queries are on {queries.device}, the bank on {bank.device}")
    k = _int_arg(k, "k", 1, most)
    if metric not in METRICS:
        raise RuntimeError(f"metric must be one of {METRICS}, got {metric!r}")
    if exclude_self and queries is not bank and queries.shape != bank.shape:
        raise RuntimeError("exclude_self=True needs queries is bank, or queries of the bank's shape (row n is then bank row n)")
    return nq, m, width, k


def _classify_args(bank, bank_labels, num_classes, weights):
    if isinstance(num_classes, bool) or not isinstance(num_classes, numbers.Integral) or int(num_classes) < 1:
        raise RuntimeError(f"num_classes must be a positive integer, got {num_classes!r}")
    if weights not in ("uniform", "distance"):
        raise RuntimeError(f"weights must be 'uniform' or 'distance', got {weights!r}")
    if (not isinstance(bank_labels, torch.Tensor) or bank_labels.dim() != 1 or bank_labels.dtype.is_floating_point
            or bank_labels.dtype.is_complex or bank_labels.dtype == torch.bool):
        raise RuntimeError("bank_labels must be a 1-D integer tensor, one label per bank row")
    if isinstance(bank, torch.Tensor) and bank.dim() == 2:
        if int(bank_labels.numel()) != int(bank.shape[0]):
            raise RuntimeError(f"bank_labels has {bank_labels.numel()} entries, the bank {bank.shape[0]} rows")
        if bank_labels.device != bank.device:
            raise RuntimeError(f"bank_labels are on {bank_labels.device}, the bank on {bank.device}")
    return int(num_classes)


# ---------------------------------------------------------------------------------------------------- the C call
def _search(queries, bank, k, self_offset=-1):
    """`eae_knn_search` on contiguous fp32 device tensors: (idx, dist)."""
    nq, width = queries.shape
    m = bank.shape[0]
    lib = _lib.load()
    idx = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
    nbytes = lib.eae_knn_workspace_bytes(nq, m, width, k)
    ws = _alloc_workspace(nbytes, queries.device, or_none=True)
    with torch.cuda.device(queries.device):
        check(lib.eae_knn_search(_stream(), _ptr(queries), nq, _ptr(bank), m, width, k, int(self_offset), _ptr(idx), _ptr(dist), _ptr(ws),
                                 nbytes))
    return idx, dist


def _unit_rows(t):
    """Rows scaled to unit length, out of place.  A zero row becomes NaN (0 / 0): it has no direction and is treated as non-finite."""
    return (t / t.norm(dim=1, keepdim=True)).contiguous()


def _knn(queries, bank, k, self_offset, metric):
    if metric == "cosine":
        same = queries is bank
        bank = _unit_rows(bank)
        queries = bank if same else _unit_rows(queries)
        idx, dist = _search(queries, bank, k, self_offset)
        return idx, dist * 0.5                      # unit rows: d^2 = 2 - 2 cos
    return _search(queries.contiguous(), bank.contiguous(), k, self_offset)


# ---------------------------------------------------------------------------------------------------- public functions
def knn_search(queries, bank, k, exclude_self=False, metric="l2"):
    """`KNNResult`: for every row of queries [Nq, L] the k nearest rows of bank [M, L], compared in fp32 as
    ||b||^2 - 2 q.b; equal scores in ascending bank index.  No Nq x M matrix is made.

    exclude_self: row n may not match bank row n (leave-one-out): needs ``queries is bank`` or equal shapes.
    metric: "l2" (dist = squared distance) or "cosine" (both sides are scaled to unit rows first, out of place; dist = 1 - cos; a zero
    row has no direction and counts as non-finite: as a query it gets -1 / NaN, as a bank row it is never returned)."""
    _, _, _, k = _search_args(queries, bank, k, exclude_self, metric)
    _require_gpu(queries.device)
    return KNNResult(*_knn(queries, bank, k, 0 if exclude_self else -1, metric))


def _vote(idx, dist, bank_labels, num_classes, weights):
    """(labels [Nq], votes [Nq, C]) from a search result: gather the neighbours' labels, add their votes class by class.  The votes of
    neighbour j are added in the j-th of k scatter_add_ calls, each of which adds at most once to an element: the sums are in
    neighbour order and repeatable."""
    nq, k = idx.shape
    valid = idx >= 0
    lab = bank_labels.to(torch.int64)[idx.clamp(min=0)]
    valid &= (lab >= 0) & (lab < num_classes)
    slot = torch.where(valid, lab, num_classes)                        # what casts no vote lands in a slot that is dropped
    w = torch.ones_like(dist) if weights == "uniform" else 1.0 / (dist + 1e-12)
    w = torch.where(valid, w, 0.0)
    acc = torch.zeros((nq, num_classes + 1), dtype=torch.float32, device=idx.device)
    for j in range(k):
        acc.scatter_add_(1, slot[:, j:j + 1], w[:, j:j + 1])
    votes = acc[:, :num_classes].contiguous()
    first = votes.argmax(dim=1)                                        # torch returns the first maximum: the lowest class id on a tie
    labels = torch.where(valid.any(dim=1), first, -1)
    return labels, votes


def knn_classify(queries, bank, bank_labels, k, num_classes, weights="uniform", exclude_self=False, metric="l2"):
    """(labels [Nq] int64, votes [Nq, num_classes] float32): kNN classification from a labelled bank.  votes counts the labels of the
    neighbours `knn_search` returns; ``weights="distance"`` weights each neighbour by 1 / (dist + 1e-12) instead, summed in neighbour
    order.  A neighbour slot of -1, or a bank label outside [0, num_classes) (an unlabelled row), casts no vote.  The label is the class
    with the most votes, the lowest class id on a tie; a row with no vote gets -1."""
    _, _, _, k = _search_args(queries, bank, k, exclude_self, metric)
    num_classes = _classify_args(bank, bank_labels, num_classes, weights)
    _require_gpu(queries.device)
    idx, dist = _knn(queries, bank, k, 0 if exclude_self else -1, metric)
    return _vote(idx, dist, bank_labels, num_classes, weights)


# ---------------------------------------------------------------------------------------------------- scenes
def similar_windows(scene, encoder, query, k, divisor=1.0, stride=None, batch=512, nodata=None, mask=None, max_invalid=0.0, rule="all",
                    windows=None, border=None, fill=0, anchor="center", metric="l2"):
    """`KNNResult` of window ids: query by example on a scene.  The window set is taken as `cluster_scene` takes it (the whole grid,
    the ids in ``windows=``, or under ``nodata=`` / ``mask=`` the valid windows) and encoded once, as `encode_scene` encodes it; the
    latents are the bank.  idx [Nq, k] holds window ids of the grid (row-major, as `window_grid` numbers them), -1 in an empty slot.

    query: a 1-D int64 tensor of window ids -- each must belong to the window set (checked with one host readback); their latents
    come from the same pass, a query is never its own neighbour, and k is at most 31 (the search asks for k + 1 and drops the query's
    own entry) -- or a float32 [Nq, L] tensor of latents (L = the encoder's latent_dim), searched as they are."""
    h = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, allow_empty=False, border=border,
                   fill=fill, anchor=anchor)
    n_grid, width = h.n_h * h.n_w, int(h.enc.latent_dim)
    if metric not in METRICS:
        raise RuntimeError(f"metric must be one of {METRICS}, got {metric!r}")
    by_id = isinstance(query, torch.Tensor) and query.dim() == 1 and query.dtype == torch.int64
    if by_id:
        k = _int_arg(k, "k", 1, MAX_K - 1)
        if query.numel() == 0:
            raise RuntimeError("query is empty")
        if query.device != scene.device:
            raise RuntimeError(f"query is on {query.device}, the scene on {scene.device}")
        if bool(((query < 0) | (query >= n_grid)).any()):
            raise RuntimeError(f"query holds a window id outside the {h.n_h} x {h.n_w} grid")
    else:
        k = _int_arg(k, "k", 1, MAX_K)
        if _rows_arg(query, "query")[1] != width:
            raise RuntimeError(f"query latents have width {query.shape[1]}, the encoder's latent_dim is {width}")
        if query.device != scene.device:
            raise RuntimeError(f"query is on {query.device}, the scene on {scene.device}")
    ids, z = _scene_latents(h)
    if not by_id:
        idx, dist = _knn(query, z, k, -1, metric)
    else:
        pos = query
        if ids is not None:
            pos = h.scatter(ids, torch.arange(ids.numel(), device=z.device), -1, flat=True)[query]       # window id -> row of z
            if bool((pos < 0).any()):
                raise RuntimeError("query holds a window id that is not in the window set")
        idx1, dist1 = _knn(z[pos].contiguous(), z, k + 1, -1, metric)
        own = idx1 == pos[:, None]
        drop = torch.where(own.any(dim=1), own.to(torch.int8).argmax(dim=1), k)      # the own entry, or (it lies beyond) the last
        col = torch.arange(k, device=z.device)[None, :]
        col = col + (col >= drop[:, None]).to(torch.int64)
        idx, dist = idx1.gather(1, col), dist1.gather(1, col)
    if ids is not None:
        idx = torch.where(idx >= 0, ids[idx.clamp(min=0)], -1)
    return KNNResult(idx, dist)


def knn_classify_scene(scene, encoder, bank, bank_labels, k, num_classes, weights="uniform", divisor=1.0, stride=None, batch=512,
                       nodata=None, mask=None, max_invalid=0.0, rule="all", windows=None, border=None, fill=0, anchor="center",
                       metric="l2"):
    """(label_map int64 [nH, nW], votes float32 [num_classes, nH, nW]): the class map of a scene by `knn_classify` of its windows'
    latents (`encode_scene`, with `cluster_scene`'s window selection) against a labelled bank [M, L], L = the encoder's latent_dim.
    Windows that are not run hold -1 and 0 votes, as does a window with no vote."""
    h = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, allow_empty=False, border=border,
                   fill=fill, anchor=anchor)
    if _rows_arg(bank, "bank")[1] != int(h.enc.latent_dim):
        raise RuntimeError(f"the bank has width {bank.shape[1]}, the encoder's latent_dim is {int(h.enc.latent_dim)}")
    if bank.device != scene.device:
        raise RuntimeError(f"the bank is on {bank.device}, the scene on {scene.device}")
    k = _int_arg(k, "k", 1, MAX_K)
    if metric not in METRICS:
        raise RuntimeError(f"metric must be one of {METRICS}, got {metric!r}")
    num_classes = _classify_args(bank, bank_labels, num_classes, weights)
    ids, z = _scene_latents(h)
    labels, votes = knn_classify(z, bank, bank_labels, k, num_classes, weights=weights, metric=metric)
    return h.scatter(ids, labels, -1), h.scatter(ids, votes, 0.0, channels_first=True)
