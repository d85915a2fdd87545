"""Gaussian maximum-likelihood classification of latents on the device: the supervised baseline of remote sensing, on the rows
`encode_scene` returns.

A mean and a covariance are fitted to every class, and a row goes to the class with the smallest discriminant

    score_k(z) = (z - mu_k)^T Sigma_k^-1 (z - mu_k) + log det Sigma_k - 2 log pi_k .

The two hot kernels are entry points of the C library (include/eae.h, "latent Gaussian models"):
`eae_class_scatter` (per-class scatter matrices about given means, fixed-order partial sums: bitwise symmetric and repeatable) and
`eae_gauss_score` (per-class quadratic forms ||W_k^T (z - mu_k)||^2 in exact fp32 on the f32-input MFMA, running argmin in registers:
no N x K x L temporary).  Everything here takes fp32 latents z [N, L] (on a HIP device), 1 <= L <= 256, 1 <= K <= 256; labels are
int64 with -1 for a row that holds a NaN or an Inf.  There is no optimiser and no seed: the same data give the same model, bit for bit.

- `class_scatter` is the moments: counts, means and scatter matrices of labelled rows;
- `gaussian_fit` turns them into a `GaussianModel` (covariances, shrinkage, Cholesky whitening and priors on the host in float64);
- `gaussian_predict` is one score call: labels, squared Mahalanobis distances and on request log-posteriors;
- `gaussian_classify_scene` is the class map of a scene with a distance map that serves as a reject map;
- `scatter_axes` derives 2-D views of the latent space from the moments: principal axes or Fisher's discriminant axes.
"""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check
from ._args import _alloc_workspace, _int_arg, _rows_arg
from .cluster import MAX_K, _predict, _update, _workspace
from .engine import _ptr, _stream, _require_gpu

COVARIANCES = ("full", "tied")


class GaussianModel(NamedTuple):
    """means [K,L] float32; whiten float32 [K,L,L] ("full") or [1,L,L] ("tied"): W = C^-T of the Cholesky factor Sigma = C C^T, so that
    ||W^T (z - mu)||^2 is the squared Mahalanobis distance; offset [K] float32 = logdet - 2 log prior, +inf for an absent class (fewer
    than 2 rows, or prior 0); counts [K] int64; logdet [K] float64 (+inf for an absent class); covariance and reg as given."""
    means: torch.Tensor
    whiten: torch.Tensor
    offset: torch.Tensor
    counts: torch.Tensor
    logdet: torch.Tensor
    covariance: str
    reg: float


# ---------------------------------------------------------------------------------------------------- host-side validation
def _labels_arg(labels, z, what="labels"):
    if (not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype.is_complex
            or labels.dtype == torch.bool):
        raise RuntimeError(f"{what} must be a 1-D integer tensor, one label per row of z")
    if int(labels.numel()) != int(z.shape[0]):
        raise RuntimeError(f"{what} has {labels.numel()} entries, z {z.shape[0]} rows")
    if labels.device != z.device:
        raise RuntimeError(f"{what} are on {labels.device}, z on {z.device}")


def _model_args(covariance, reg, priors, k):
    if covariance not in COVARIANCES:
        raise RuntimeError(f"covariance must be one of {COVARIANCES}, got {covariance!r}")
    if isinstance(reg, bool) or not isinstance(reg, numbers.Real) or not 0.0 <= float(reg) <= 1.0:
        raise RuntimeError(f"reg must be a number in [0, 1], got {reg!r}")
    if isinstance(priors, torch.Tensor):
        if priors.dim() != 1 or int(priors.numel()) != k or not priors.dtype.is_floating_point:
            raise RuntimeError(f"priors must be 'empirical', 'uniform' or a floating-point tensor [{k}], one entry per class")
        p = priors.detach().to(device="cpu", dtype=torch.float64)
        if not bool(torch.isfinite(p).all()) or bool((p < 0).any()) or not bool((p > 0).any()):
            raise RuntimeError("priors must be finite and >= 0, and not all zero")
    elif priors not in ("empirical", "uniform"):
        raise RuntimeError(f"priors must be 'empirical', 'uniform' or a [K] tensor, got {priors!r}")


def _moments_arg(counts, means, scatter):
    """(K, L) of counts [K] integer, means [K, L] and scatter [K, L, L] floating point."""
    if not isinstance(means, torch.Tensor) or means.dim() != 2 or not means.dtype.is_floating_point:
        raise RuntimeError("means must be a floating-point tensor [K, L]")
    k, width = int(means.shape[0]), int(means.shape[1])
    if k < 1 or width < 1:
        raise RuntimeError(f"means must have at least one class and one column, got {tuple(means.shape)}")
    if not isinstance(counts, torch.Tensor) or counts.dtype.is_floating_point or counts.dtype == torch.bool or tuple(counts.shape) != (k,):
        raise RuntimeError(f"counts must be an integer tensor [{k}], one entry per row of means")
    if not isinstance(scatter, torch.Tensor) or not scatter.dtype.is_floating_point or tuple(scatter.shape) != (k, width, width):
        raise RuntimeError(f"scatter must be a floating-point tensor [{k}, {width}, {width}]")
    return k, width


def _model_arg(model, width, device):
    if not isinstance(model, GaussianModel):
        raise RuntimeError(f"model must be a GaussianModel (gaussian_fit returns one), got {type(model).__name__}")
    k, mwidth = _rows_arg(model.means, "model.means", "[K, L]", MAX_K)
    if mwidth != int(width):
        raise RuntimeError(f"the model has width {mwidth}, the latents {width}")
    w, off = model.whiten, model.offset
    if (not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 3 or int(w.shape[0]) not in (1, k)
            or tuple(w.shape[1:]) != (mwidth, mwidth)):
        raise RuntimeError(f"model.whiten must be a float32 tensor [{k} or 1, {mwidth}, {mwidth}]")
    if not isinstance(off, torch.Tensor) or off.dtype != torch.float32 or tuple(off.shape) != (k,):
        raise RuntimeError(f"model.offset must be a float32 tensor [{k}]")
    for t, name in ((model.means, "means"), (w, "whiten"), (off, "offset")):
        if t.device != device:
            raise RuntimeError(f"model.{name} is on {t.device}, the latents on {device}")
    return k


def _reject_arg(reject):
    if reject is None:
        return None
    if isinstance(reject, bool) or not isinstance(reject, numbers.Real) or math.isnan(float(reject)) or float(reject) < 0.0:
        raise RuntimeError(f"reject must be None or a squared distance >= 0, got {reject!r}")
    return float(reject)


# ---------------------------------------------------------------------------------------------------- the C calls
def _moments(z, labels, k):
    """(counts, means, scatter) of contiguous fp32 device rows: the rows are grouped by class with one stable sort, counts and means are
    `eae_kmeans_update` on a zeroed centroid buffer (an empty class keeps its zeros), the scatter is `eae_class_scatter` about them."""
    n, width = z.shape
    lib = _lib.load()
    dev = z.device
    lab = labels.to(torch.int64)
    # a row with a NaN or an Inf: NaN distance to the origin from `eae_kmeans_assign`, as `kmeans_init` finds them (no N x L temporary)
    finite = ~torch.isnan(_predict(z, torch.zeros((1, width), dtype=torch.float32, device=dev))[1])
    key = torch.where((lab >= 0) & (lab < k) & finite, lab, k)         # what is not summed sorts into a tail no segment covers
    order = torch.sort(key, stable=True)[1]
    means = torch.zeros((k, width), dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    scatter = torch.empty((k, width, width), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _update(z, key, means, counts, _workspace(z, k))
        seg = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)))
        ws = _alloc_workspace(lib.eae_class_scatter_workspace_bytes(n, width, k), dev)
        check(lib.eae_class_scatter(_stream(), _ptr(z), n, width, _ptr(key), _ptr(order), _ptr(seg), k, _ptr(means), _ptr(scatter),
                                    _ptr(ws), ws.numel()))
    return counts, means, scatter


def _score(z, model, want_scores=False):
    """`eae_gauss_score` on contiguous fp32 device rows: (labels, maha, scores or None)."""
    n, width = z.shape
    k = int(model.means.shape[0])
    dev = z.device
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    maha = torch.empty(n, dtype=torch.float32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev) if want_scores else None
    mu, w, off = model.means.contiguous(), model.whiten.contiguous(), model.offset.contiguous()
    stride = width * width if int(w.shape[0]) == k and k > 1 else 0
    with torch.cuda.device(dev):
        check(_lib.load().eae_gauss_score(_stream(), _ptr(z), n, width, _ptr(mu), _ptr(w), stride, _ptr(off), k, _ptr(labels),
                                          _ptr(maha), None, _ptr(scores)))
    return labels, maha, scores


# ---------------------------------------------------------------------------------------------------- the host part of the fit
def _fit_from_moments(counts, means, scatter, covariance="full", reg=1e-3, priors="empirical"):
    """`GaussianModel` on the host from the moments of `class_scatter`, in float64; needs neither the library nor a device.

    A class with fewer than 2 rows is absent: offset +inf, logdet +inf, a zero whitening matrix, left out of the tied pool and of the
    priors' normalisation.  Sigma_k = S_k / (n_k - 1) ("full") or Sigma = sum S_k / (N_labelled - K_present) ("tied"), shrunk as
    (1 - reg) Sigma + reg (tr Sigma / L) I; Sigma = C C^T, W = C^-T, logdet = 2 sum log diag C; offset = logdet - 2 log pi."""
    k, width = _moments_arg(counts, means, scatter)
    _model_args(covariance, reg, priors, k)
    reg = float(reg)
    n = counts.detach().to(device="cpu", dtype=torch.int64)
    s = scatter.detach().to(device="cpu", dtype=torch.float64)
    present = n >= 2
    eye = torch.eye(width, dtype=torch.float64)

    def whitening(cov, who):
        cov = (1.0 - reg) * cov + reg * (torch.trace(cov) / width) * eye
        c, info = torch.linalg.cholesky_ex(cov)
        if int(info) != 0 or not bool(torch.isfinite(c).all()):
            raise RuntimeError(f"the covariance of {who} is not positive definite: the Cholesky factorisation failed (fewer distinct "
                               f"rows than the latent width {width}? raise reg, now {reg})")
        w = torch.linalg.solve_triangular(c, eye, upper=False).T
        return w, 2.0 * torch.log(torch.diagonal(c)).sum()

    logdet = torch.full((k,), math.inf, dtype=torch.float64)
    if covariance == "full":
        whiten = torch.zeros((k, width, width), dtype=torch.float64)
        for q in torch.nonzero(present).flatten().tolist():
            whiten[q], logdet[q] = whitening(s[q] / float(n[q] - 1), f"class {q}")
    else:
        whiten = torch.zeros((1, width, width), dtype=torch.float64)
        if bool(present.any()):
            pooled = s[present].sum(0) / float(n[present].sum() - present.sum())
            whiten[0], ld = whitening(pooled, "the tied model (all classes pooled)")
            logdet[present] = ld

    if isinstance(priors, torch.Tensor):
        pi = priors.detach().to(device="cpu", dtype=torch.float64).clone()
    elif priors == "uniform":
        pi = torch.ones(k, dtype=torch.float64)
    else:
        pi = n.to(torch.float64)
    pi[~present] = 0.0
    if bool(present.any()):
        if not float(pi.sum()) > 0.0:
            raise RuntimeError("priors are zero for every class that has rows")
        pi = pi / pi.sum()
    offset = torch.where(pi > 0, logdet - 2.0 * torch.log(pi), math.inf)
    return GaussianModel(means.detach().to(device="cpu", dtype=torch.float32), whiten.to(torch.float32), offset.to(torch.float32), n,
                         logdet, covariance, reg)


# ---------------------------------------------------------------------------------------------------- public functions
def class_scatter(z, labels, num_classes):
    """(counts [K] int64, means [K,L] float32, scatter [K,L,L] float32) of the rows of z [N, L] by label: scatter[k] = sum over the rows
    of class k of (z - mean_k)(z - mean_k)^T, centred in fp32 before the product.  Labels outside [0, K) are skipped, and a row that
    holds a NaN or an Inf is treated as unlabelled.  A class without rows has count 0, a zero mean and a zero matrix.  Every matrix is
    bitwise symmetric, and the result is bitwise the same from run to run (no float atomics).  Nothing is read back."""
    _rows_arg(z, "z", "[N, L]")
    k = _int_arg(num_classes, "num_classes", 1, MAX_K)
    _labels_arg(labels, z)
    _require_gpu(z.device)
    return _moments(z.contiguous(), labels, k)


def gaussian_fit(z, labels, num_classes, covariance="full", reg=1e-3, priors="empirical"):
    """`GaussianModel` of the labelled rows of z [N, L]: one pass of `class_scatter` on the device, then the K small factorisations on
    the host in float64 (one readback of the moments).

    covariance: "full" (a covariance a class: quadratic boundaries) or "tied" (one pooled covariance: linear boundaries).
    reg: shrinkage towards a sphere, Sigma <- (1 - reg) Sigma + reg (tr Sigma / L) I; with 0 a class needs more distinct rows than L.
    priors: "empirical" (the class frequencies), "uniform", or a [K] tensor; normalised over the classes that are present.
    A class with fewer than 2 rows is absent and is never predicted.  A covariance that is not positive definite raises an error
    that names the class."""
    _rows_arg(z, "z", "[N, L]")
    k = _int_arg(num_classes, "num_classes", 1, MAX_K)
    _labels_arg(labels, z)
    _model_args(covariance, reg, priors, k)
    _require_gpu(z.device)
    counts, means, scatter = _moments(z.contiguous(), labels, k)
    m = _fit_from_moments(counts.cpu(), means.cpu(), scatter.cpu(), covariance, reg, priors)
    dev = z.device
    return GaussianModel(means, m.whiten.to(dev), m.offset.to(dev), counts, m.logdet.to(dev), m.covariance, m.reg)


def gaussian_predict(z, model, posteriors=False):
    """(labels int64 [N], maha float32 [N]): the class with the smallest score of every row and the squared Mahalanobis distance to it,
    in fp32; the lowest class wins a tie; a row with a NaN or an Inf gets -1 and NaN, as does every row when no class is present.
    Under the model maha follows a chi-square law with L degrees of freedom.  posteriors=True adds log-posteriors float32 [N, K]:
    -score / 2 minus its logsumexp over the present classes (-inf for an absent class, NaN for a -1 row)."""
    _, width = _rows_arg(z, "z", "[N, L]")
    _model_arg(model, width, z.device)
    if not isinstance(posteriors, bool):
        raise RuntimeError(f"posteriors must be True or False, got {posteriors!r}")
    _require_gpu(z.device)
    labels, maha, scores = _score(z.contiguous(), model, want_scores=posteriors)
    if not posteriors:
        return labels, maha
    half = (scores - scores.min(dim=1, keepdim=True).values) * -0.5          # 0 for the chosen class: nothing large is exponentiated
    return labels, maha, half - torch.logsumexp(half, dim=1, keepdim=True)


def gaussian_classify_scene(scene, encoder, model, reject=None, divisor=1.0, stride=None, batch=512, nodata=None, mask=None,
                            max_invalid=0.0, rule="all", windows=None, border=None, fill=0, anchor="center"):
    """(label_map int64 [nH, nW], maha_map float32 [nH, nW]): the class map of a scene by `gaussian_predict` of its windows' latents
    (`encode_scene`, with `cluster_scene`'s window selection), L = the encoder's latent_dim.  Windows that are not run hold -1 and NaN.

    maha_map is the squared Mahalanobis distance of every window to its class: under the model it follows a chi-square law with L
    degrees of freedom, so a window far in that law's tail looks like none of the training classes.  reject=t sets the label of every
    window with maha > t to -1 and keeps its distance (for instance t = the 0.99 quantile of chi-square with L degrees of freedom)."""
    from .scene import _host_plan, _scene_latents
    h = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, allow_empty=False, border=border,
                   fill=fill, anchor=anchor)
    _model_arg(model, int(h.enc.latent_dim), scene.device)
    reject = _reject_arg(reject)
    ids, z = _scene_latents(h)
    labels, maha, _ = _score(z, model)
    if reject is not None:
        labels = torch.where(maha > reject, -1, labels)
    return h.scatter(ids, labels, -1), h.scatter(ids, maha, math.nan)


def scatter_axes(counts, means, scatter, kind="lda", n_components=2):
    """(origin [L], axes [L, n], values [n]), float64 on the device of `means`: a low-dimensional view (z - origin) @ axes of the
    latent space from the moments of `class_scatter`, computed on the host in float64.  origin is the mean of all labelled rows.
    With S_w = sum_k S_k (within) and S_b = sum_k n_k (m_k - origin)(m_k - origin)^T (between):

    kind="pca": the leading eigenvectors of the total scatter S_w + S_b, orthonormal; values = its eigenvalues (the squared singular
    values of the centred rows), descending.
    kind="lda": Fisher's axes, the generalised eigenvectors S_b v = lambda S_w v with the largest lambda, scaled to v^T S_w v = 1;
    values = lambda (at most K - 1 are non-zero).  S_w must be positive definite."""
    k, width = _moments_arg(counts, means, scatter)
    if kind not in ("lda", "pca"):
        raise RuntimeError(f"kind must be 'lda' or 'pca', got {kind!r}")
    nc = _int_arg(n_components, "n_components", 1, width)
    n = counts.detach().to(device="cpu", dtype=torch.float64)
    if not float(n.sum()) > 0.0:
        raise RuntimeError("no labelled row: every count is zero")
    m = means.detach().to(device="cpu", dtype=torch.float64)
    origin = (n[:, None] * m).sum(0) / n.sum()
    dm = m - origin
    sw = scatter.detach().to(device="cpu", dtype=torch.float64).sum(0)
    sb = (n[:, None, None] * dm[:, :, None] * dm[:, None, :]).sum(0)
    if kind == "pca":
        vals, vecs = torch.linalg.eigh(sw + sb)
    else:
        c, info = torch.linalg.cholesky_ex(sw)
        if int(info) != 0:
            raise RuntimeError("the within-class scatter is not positive definite: kind='lda' needs more labelled rows than the "
                               "latent width")
        ci = torch.linalg.solve_triangular(c, torch.eye(width, dtype=torch.float64), upper=False)
        mid = ci @ sb @ ci.T
        vals, y = torch.linalg.eigh((mid + mid.T) * 0.5)
        vecs = ci.T @ y
    top = torch.arange(width - 1, width - 1 - nc, -1)
    dev = means.device
    return origin.to(dev), vecs[:, top].contiguous().to(dev), vals[top].contiguous().to(dev)
