"""Change detection between two scenes of one place: IR-MAD on the device, and post-classification comparison.

The iteratively reweighted multivariate alteration detection (IR-MAD, Nielsen 2007) finds the pairs of linear combinations a_i^T x and
b_i^T y of the two dates' bands with the highest correlations rho_i (canonical correlation analysis); the differences of the pairs,
the MAD variates, are invariant to affine changes of either date's bands (gain, offset, band mixing), so two dates with different
illumination compare without a radiometric correction.  Scaled to unit variance their sum of squares Z follows a chi-square law with
C degrees of freedom where nothing changed; the iteration weights every pixel by that law's survival probability and repeats, so the
statistics settle on the pixels that did not change.  The two passes over the scenes are kernels of the C library (include/eae.h,
"change detection"); the C x C solve runs on the host in float64.

Conventions: x = a / divisor_a and y = b / divisor_b per band; the pairs come in descending order of rho (the first variate is the
most stable combination, the last carries the most change); the sign of pair i makes the largest-magnitude entry of Sxx a_i positive;
a_i^T Sxx a_i = b_i^T Syy b_i = 1; sigma_i = sqrt(2 (1 - rho_i)), not below `SIGMA_FLOOR`; variate_i = (a_i^T (x - mean_a) - b_i^T
(y - mean_b)) / sigma_i.  The scenes must be co-registered and have the same number of bands; `register.coregister` brings a scene
that is not aligned onto the other's grid and returns the validity raster that ``mask=~valid`` takes.

- `joint_moments`: weighted mean and covariance of the stacked pixel vector [x, y], one pass;
- `mad_from_moments`: the canonical-correlation solve, host only;
- `mad_fit`: the iteration; `mad_transform`: chi2, prob and variates of a fitted model;
- `detect_change`: fit, transform, calibrated change mask;
- `invariant_regression`: per-band gain and offset between the dates from the pixels that did not change;
- `class_transitions`: the from-to table of two class maps (`report.transition_table` prints it).
"""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _int_arg
from .engine import _ptr, _stream, _require_gpu

MAX_BANDS = 16
_PIXEL_LIMIT = 2 ** 31
SIGMA_FLOOR = 1e-6            # lowest sigma_i: a pair correlated to within 5e-13 of 1 would otherwise divide by (nearly) zero
_PIVOT_FLOOR = 1e-12          # a Cholesky pivot below this share of its band's variance is rounding noise: the factorisation failed
_PIVOT_STEP = 16              # the default pivot is the mean of every 16th pixel of every 16th row


class JointMoments(NamedTuple):
    """n: the sum of the weights; mean float64 [2C] and cov float64 [2C, 2C] (NumPy, weighted, divided by n) of [x, y]; count: the
    number of valid pixels.  With n == 0 mean and cov are NaN."""
    n: float
    mean: np.ndarray
    cov: np.ndarray
    count: int


class MadModel(NamedTuple):
    """rho [C] descending; a, b [C, C]: column i is pair i; mean_a, mean_b [C]; sigma [C]; all float64 NumPy.  iterations: how many
    `mad_fit` ran; history: rho of every iteration."""
    rho: np.ndarray
    a: np.ndarray
    b: np.ndarray
    mean_a: np.ndarray
    mean_b: np.ndarray
    sigma: np.ndarray
    iterations: int
    history: tuple


class ChangeResult(NamedTuple):
    """chi2, prob float32 [H, W] and change bool [H, W] on the device (chi2 NaN, prob 0, change False for an invalid pixel); scale:
    what chi2 was divided by before the test (1.0 without calibration); model: the `MadModel`."""
    chi2: torch.Tensor
    prob: torch.Tensor
    change: torch.Tensor
    scale: float
    model: MadModel


class _Pair(NamedTuple):
    a: torch.Tensor
    b: torch.Tensor
    div_a: torch.Tensor          # fp32 [C], wherever the caller's divisor was
    div_b: torch.Tensor
    nodata_a: tuple              # (mode, value, rule id)
    nodata_b: tuple
    mask: object                 # uint8 [H, W] or None
    weights: object              # fp32 [H, W] or None


# ---------------------------------------------------------------------------------------------------- host-side validation
def _divisor_arg(divisor, c, name):
    div = torch.as_tensor(divisor, dtype=torch.float32).reshape(-1)
    if div.numel() == 1:
        div = div.expand(c)
    if div.numel() != c:
        raise RuntimeError(f"{name} must have one value per band ({c}), got {div.numel()}")
    return div


def _host_args(a, b, divisor_a=1.0, divisor_b=1.0, weights=None, nodata_a=None, nodata_b=None, mask=None, rule_a="all", rule_b="all",
               wname="weights"):
    """Every host-side check of the change functions; no device is touched."""
    from .scene import _check_scene, _mask_arg, _nodata_arg, _rule_arg
    _check_scene(a)
    _check_scene(b)
    if tuple(a.shape) != tuple(b.shape):
        raise RuntimeError(f"the two scenes must have one shape, got {list(a.shape)} and {list(b.shape)}")
    if a.device != b.device:
        raise RuntimeError(f"scene a is on {a.device}, scene b on {b.device}")
    c, h, w = (int(v) for v in a.shape)
    if not 1 <= c <= MAX_BANDS:
        raise RuntimeError(f"scene: the number of bands must be in 1..16, got {c}")
    if h < 1 or w < 1:
        raise RuntimeError(f"scene is empty: {[c, h, w]}")
    if h * w >= _PIXEL_LIMIT:
        raise RuntimeError(f"scene has {h} x {w} pixels: H * W must be below 2^31")
    div_a = _divisor_arg(divisor_a, c, "divisor_a")
    div_b = _divisor_arg(divisor_b, c, "divisor_b")
    nd_a = _nodata_arg(a.dtype, nodata_a) + (_rule_arg(rule_a),)
    nd_b = _nodata_arg(b.dtype, nodata_b) + (_rule_arg(rule_b),)
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or tuple(weights.shape) != (h, w):
            raise RuntimeError(f"{wname} must be a [H, W] = {[h, w]} tensor")
        if weights.dtype != torch.float32:
            raise RuntimeError(f"{wname} dtype must be float32, got {weights.dtype}")
        if weights.device != a.device:
            raise RuntimeError(f"{wname} is on {weights.device}, the scenes on {a.device}")
    return _Pair(a, b, div_a, div_b, nd_a, nd_b, _mask_arg(a, mask), weights)


def _model_arg(model, c):
    if not isinstance(model, MadModel):
        raise RuntimeError("model must be a MadModel (mad_fit or mad_from_moments)")
    if np.shape(model.a) != (c, c) or np.shape(model.b) != (c, c) or np.shape(model.sigma) != (c,) or np.shape(model.mean_a) != (c,) \
            or np.shape(model.mean_b) != (c,):
        raise RuntimeError(f"the model was fitted to {np.shape(model.sigma)[0] if np.ndim(model.sigma) == 1 else '?'} bands, the "
                           f"scenes have {c}")


def _unit_arg(v, name, lo_open=True):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (0.0 < float(v) < 1.0 if lo_open else 0.0 <= float(v) < 1.0):
        raise RuntimeError(f"{name} must be a number in {'(0, 1)' if lo_open else '[0, 1)'}, got {v!r}")
    return float(v)


def _reg_arg(reg):
    if isinstance(reg, bool) or not isinstance(reg, numbers.Real) or not 0.0 <= float(reg) <= 1.0:
        raise RuntimeError(f"reg must be a number in [0, 1], got {reg!r}")
    return float(reg)


# ---------------------------------------------------------------------------------------------------- the chi-square law on the host
def chi2_sf(dof, z):
    """Q(dof / 2, z / 2) in float64, integer dof >= 1: the closed forms the kernel evaluates in fp32."""
    h = 0.5 * float(z)
    if not h > 0.0:
        return 1.0
    m = dof // 2
    if dof % 2:
        t = math.sqrt(h) * 2.0 / math.sqrt(math.pi)
        s = 0.0
        for j in range(1, m + 1):
            if j > 1:
                t *= h / (j - 0.5)
            s += t
        return math.erfc(math.sqrt(h)) + math.exp(-h) * s
    t = s = 1.0
    for j in range(1, m):
        t *= h / j
        s += t
    return math.exp(-h) * s


def chi2_isf(dof, p):
    """z with Q(dof / 2, z / 2) = p, 0 < p < 1, by bisection (Q falls monotonically from 1 to 0)."""
    lo, hi = 0.0, 1.0
    while chi2_sf(dof, hi) > p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if chi2_sf(dof, mid) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ---------------------------------------------------------------------------------------------------- the two passes
def _scene_call_args(p, dev):
    from .scene import _DTYPES
    a, b = p.a.contiguous(), p.b.contiguous()
    c, h, w = (int(v) for v in a.shape)
    div_a, div_b = p.div_a.to(dev).contiguous(), p.div_b.to(dev).contiguous()
    keep = (a, b, div_a, div_b)
    head = (_ptr(a), _ptr(b), _DTYPES[a.dtype], _DTYPES[b.dtype], c, h, w, _ptr(div_a), _ptr(div_b), p.nodata_a[0], p.nodata_a[1],
            p.nodata_a[2], p.nodata_b[0], p.nodata_b[1], p.nodata_b[2], _ptr(p.mask))
    return keep, head, (c, h, w)


def _default_pivot(p):
    """float64 [2C]: the mean of a strided subsample of the unmasked, finite pixels (zeros when there is none)."""
    s = _PIVOT_STEP
    dev = p.a.device
    x = p.a[:, ::s, ::s].to(torch.float32) / p.div_a.to(dev)[:, None, None]
    y = p.b[:, ::s, ::s].to(torch.float32) / p.div_b.to(dev)[:, None, None]
    v = torch.cat([x, y]).reshape(x.shape[0] * 2, -1).to(torch.float64)
    ok = torch.isfinite(v).all(0)
    if p.mask is not None:
        ok &= p.mask[::s, ::s].reshape(-1) == 0
    n = int(ok.sum())
    if n == 0:
        return np.zeros(v.shape[0])
    return (v[:, ok].sum(1) / n).cpu().numpy()


def _moments(p, pivot, weights):
    """`JointMoments` of a checked pair about ``pivot`` (float64 [2C]); one read-back of 2 + 2C + (2C)^2 numbers."""
    dev = p.a.device
    _require_gpu(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        keep, head, (c, h, w) = _scene_call_args(p, dev)
        piv = torch.as_tensor(np.asarray(pivot, dtype=np.float32), device=dev).contiguous()
        if weights is not None:
            weights = weights.contiguous()
        n2 = 2 * c
        out = torch.empty(1 + n2 + n2 * n2, dtype=torch.float64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        nbytes = lib.eae_change_moments_workspace_bytes(c, h, w)
        if nbytes < 0:
            check(nbytes)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib.eae_change_moments(_stream(), *head, _ptr(weights), _ptr(piv), _ptr(out), _ptr(count), _ptr(ws), nbytes))
        m = out.cpu().numpy()
        cnt = int(count.cpu()[0])
    del keep
    n = float(m[0])
    if not n > 0.0:
        return JointMoments(n, np.full(n2, np.nan), np.full((n2, n2), np.nan), cnt)
    s = m[1:1 + n2] / n
    cov = m[1 + n2:].reshape(n2, n2) / n - np.outer(s, s)
    return JointMoments(n, piv.cpu().numpy().astype(np.float64) + s, cov, cnt)


def joint_moments(a, b, divisor_a=1.0, divisor_b=1.0, weights=None, nodata_a=None, nodata_b=None, mask=None, pivot=None, rule_a="all",
                  rule_b="all"):
    """`JointMoments` of the stacked pixel vector [x, y] over the valid pixels of two scenes [C, H, W] (uint8, uint16 or float32, the
    two dtypes may differ; C in 1..16) on one device: n = sum w, mean = sum w v / n, cov = sum w (v - mean)(v - mean)^T / n.

    ``divisor_*``: a number or one per band; ``weights``: None (1) or float32 [H, W] on the device, a NaN, negative or infinite
    weight makes its pixel invalid; ``nodata_*`` / ``rule_*`` ("all" / "any") per scene and ``mask`` as `window_invalid_counts` takes
    them; a float32 pixel with a NaN or an Inf is invalid.  The sums are taken about ``pivot`` (2C numbers; None: the mean of a
    strided subsample) in fp32 per chunk and float64 across chunks, cov = S / n - (s / n)(s / n)^T in float64 on the host: the
    pivot only has to lie near the data for the subtraction to lose nothing, and the result does not depend on it beyond rounding."""
    p = _host_args(a, b, divisor_a, divisor_b, weights, nodata_a, nodata_b, mask, rule_a, rule_b)
    c = int(a.shape[0])
    if pivot is not None:
        pivot = np.asarray(pivot.detach().cpu() if isinstance(pivot, torch.Tensor) else pivot, dtype=np.float64).reshape(-1)
        if pivot.shape[0] != 2 * c or not np.isfinite(pivot).all():
            raise RuntimeError(f"pivot must hold 2C = {2 * c} finite numbers")
    _require_gpu(a.device)
    return _moments(p, _default_pivot(p) if pivot is None else pivot, p.weights)


def mad_from_moments(m, reg=0.0):
    """`MadModel` from `JointMoments` on the host in float64; needs neither the library nor a device.

    Sxx and Syy are shrunk as (1 - reg) S + reg (tr S / C) I; Sxx = Lx Lx^T, Syy = Ly Ly^T; Lx^-1 Sxy Ly^-T = U diag(rho) V^T with rho
    descending; a = Lx^-T U, b = Ly^-T V, sigma_i = max(sqrt(2 (1 - rho_i)), SIGMA_FLOOR); pair i is negated where the
    largest-magnitude entry of Sxx a_i is negative.  A factorisation that fails, or whose pivot falls below 1e-12 of the band's
    variance (a band that is constant or a combination of the others, up to rounding), raises."""
    reg = _reg_arg(reg)
    mean, cov = np.asarray(m.mean, dtype=np.float64), np.asarray(m.cov, dtype=np.float64)
    if mean.ndim != 1 or mean.shape[0] % 2 or mean.shape[0] < 2 or cov.shape != (mean.shape[0],) * 2:
        raise RuntimeError("moments must hold mean [2C] and cov [2C, 2C]")
    if not (np.isfinite(mean).all() and np.isfinite(cov).all()):
        raise RuntimeError("the moments are not finite: no valid pixel carried a positive weight")
    c = mean.shape[0] // 2
    eye = np.eye(c)
    sxx, syy, sxy = cov[:c, :c], cov[c:, c:], cov[:c, c:]
    sxx = (1.0 - reg) * sxx + reg * (np.trace(sxx) / c) * eye
    syy = (1.0 - reg) * syy + reg * (np.trace(syy) / c) * eye
    factors = []
    for s, who in ((sxx, "a"), (syy, "b")):
        try:
            low = np.linalg.cholesky(s)
        except np.linalg.LinAlgError:
            low = None
        if low is None or not np.isfinite(low).all() or (np.diag(low) ** 2 < _PIVOT_FLOOR * np.diag(s)).any():
            raise RuntimeError(f"the band covariance of scene {who} is not positive definite: the Cholesky factorisation failed "
                               f"(constant or collinear bands? raise reg, now {reg})")
        factors.append(low)
    lx, ly = factors
    k = np.linalg.solve(lx, np.linalg.solve(ly, sxy.T).T)                 # Lx^-1 Sxy Ly^-T
    u, rho, vt = np.linalg.svd(k)
    rho = np.minimum(rho, 1.0)
    a = np.linalg.solve(lx.T, u)
    b = np.linalg.solve(ly.T, vt.T)
    t = sxx @ a
    sign = np.where(t[np.abs(t).argmax(0), np.arange(c)] < 0.0, -1.0, 1.0)
    sigma = np.maximum(np.sqrt(2.0 * (1.0 - rho)), SIGMA_FLOOR)
    return MadModel(rho, a * sign, b * sign, mean[:c].copy(), mean[c:].copy(), sigma, 0, ())


def variate_matrix(model):
    """(mean float64 [2C], T float64 [2C, C]): variates = ([x, y] - mean) @ T."""
    return (np.concatenate([model.mean_a, model.mean_b]),
            np.concatenate([model.a / model.sigma, -model.b / model.sigma]))


def _variates(p, model, want_chi2, want_prob, want_variates):
    dev = p.a.device
    _require_gpu(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        keep, head, (c, h, w) = _scene_call_args(p, dev)
        mean, t = variate_matrix(model)
        mean = torch.as_tensor(mean.astype(np.float32), device=dev).contiguous()
        t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32), device=dev)
        chi2 = torch.empty((h, w), dtype=torch.float32, device=dev) if want_chi2 else None
        prob = torch.empty((h, w), dtype=torch.float32, device=dev) if want_prob else None
        var = torch.empty((c, h, w), dtype=torch.float32, device=dev) if want_variates else None
        check(lib.eae_change_variates(_stream(), *head, _ptr(mean), _ptr(t), c, _ptr(chi2), _ptr(prob), _ptr(var)))
    del keep
    return chi2, prob, var


def _fit(p, max_iter, tol, reg):
    _require_gpu(p.a.device)
    weights, pivot, history, model = p.weights, _default_pivot(p), [], None
    for it in range(max_iter):
        m = _moments(p, pivot, weights)
        model = mad_from_moments(m, reg)
        history.append(model.rho.copy())
        if it > 0 and float(np.abs(history[-1] - history[-2]).max()) < tol:
            break
        if it + 1 < max_iter:
            _, weights, _ = _variates(p, model, False, True, False)
            pivot = m.mean
    return model._replace(iterations=len(history), history=tuple(history))


def _fit_args(max_iter, tol, reg):
    max_iter = _int_arg(max_iter, "max_iter", 1, 2 ** 31 - 1)
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not float(tol) >= 0.0:
        raise RuntimeError(f"tol must be a number >= 0, got {tol!r}")
    return max_iter, float(tol), _reg_arg(reg)


def mad_fit(a, b, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask=None, max_iter=30, tol=1e-3, reg=0.0, rule_a="all",
            rule_b="all"):
    """IR-MAD: a `MadModel` of two scenes (arguments as `joint_moments`).  Iteration 0 weights every valid pixel 1; iteration t
    weights it by prob of iteration t - 1's model and takes that iteration's mean as the pivot.  Stops after ``max_iter`` iterations
    or when no rho moved by ``tol`` or more; max_iter=1 is plain MAD.  ``history`` keeps rho of every iteration.  An iteration is two
    passes over the scenes and one small read-back; the only raster it allocates is the weights'."""
    max_iter, tol, reg = _fit_args(max_iter, tol, reg)
    return _fit(_host_args(a, b, divisor_a, divisor_b, None, nodata_a, nodata_b, mask, rule_a, rule_b), max_iter, tol, reg)


def mad_transform(a, b, model, variates=False, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask=None, rule_a="all",
                  rule_b="all"):
    """(chi2 float32 [H, W], prob float32 [H, W], variates float32 [C, H, W] or None) on the device: the MAD variates of every pixel
    under ``model``, their sum of squares and its chi-square survival probability with C degrees of freedom (the no-change
    probability).  An invalid pixel gets NaN, 0 and NaN."""
    p = _host_args(a, b, divisor_a, divisor_b, None, nodata_a, nodata_b, mask, rule_a, rule_b)
    _model_arg(model, int(a.shape[0]))
    if not isinstance(variates, bool):
        raise RuntimeError(f"variates must be True or False, got {variates!r}")
    return _variates(p, model, True, True, variates)


def detect_change(a, b, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask=None, max_iter=30, tol=1e-3, reg=0.0,
                  alpha=0.01, calibrate=True, rule_a="all", rule_b="all"):
    """`ChangeResult` of two scenes: `mad_fit`, `mad_transform`, and the mask of the pixels whose no-change probability is below
    ``alpha``.

    The iteration's weights shrink the variance of the no-change pixels, so chi2 of an unchanged pixel is larger than a chi-square
    variable and the raw prob flags far more than ``alpha`` of them.  calibrate=True divides chi2 by scale = median(chi2 over the
    valid pixels) / median of the chi-square law with C degrees of freedom before the test, which assumes that FEWER THAN HALF of the
    valid pixels changed (the median is then a no-change pixel's).  calibrate=False tests the raw prob (scale = 1).  ``chi2`` and
    ``prob`` are returned as the kernel wrote them, unscaled."""
    max_iter, tol, reg = _fit_args(max_iter, tol, reg)
    alpha = _unit_arg(alpha, "alpha")
    if not isinstance(calibrate, bool):
        raise RuntimeError(f"calibrate must be True or False, got {calibrate!r}")
    p = _host_args(a, b, divisor_a, divisor_b, None, nodata_a, nodata_b, mask, rule_a, rule_b)
    model = _fit(p, max_iter, tol, reg)
    chi2, prob, _ = _variates(p, model, True, True, False)
    c = int(a.shape[0])
    scale = 1.0
    if calibrate:
        med = float(chi2.reshape(-1).nanmedian())
        if math.isfinite(med) and med > 0.0:
            scale = med / chi2_isf(c, 0.5)
        change = chi2 > scale * chi2_isf(c, alpha)                       # Q(chi2 / scale) < alpha; False for NaN
    else:
        change = (prob < alpha) & ~torch.isnan(chi2)
    return ChangeResult(chi2, prob, change, scale, model)


def invariant_regression(a, b, prob, threshold=0.95, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask=None, rule_a="all",
                         rule_b="all"):
    """(gain float64 [C], offset float64 [C], count): the orthogonal regression y_c = gain_c x_c + offset_c of every band over the
    invariant pixels, those with prob > threshold (``prob``: float32 [H, W], `mad_transform`'s or `detect_change`'s); count is how
    many there are.  (y - offset) / gain normalises scene b to scene a's radiometry.  One `joint_moments` pass with the 0 / 1 weights;
    band c's line comes from its 2 x 2 block of cov: gain = (syy - sxx + sqrt((syy - sxx)^2 + 4 sxy^2)) / (2 sxy)."""
    threshold = _unit_arg(threshold, "threshold", lo_open=False)
    if prob is None:
        raise RuntimeError("prob must be a [H, W] float32 tensor")
    p = _host_args(a, b, divisor_a, divisor_b, prob, nodata_a, nodata_b, mask, rule_a, rule_b, wname="prob")
    _require_gpu(a.device)
    w = (prob > threshold).to(torch.float32)
    m = _moments(p, _default_pivot(p), w)
    c = int(a.shape[0])
    count = int(round(m.n))
    if count < 2:
        raise RuntimeError(f"{count} pixels have prob > {threshold}: too few for a regression")
    idx = np.arange(c)
    sxx, syy, sxy = m.cov[idx, idx], m.cov[c + idx, c + idx], m.cov[idx, c + idx]
    if (sxy == 0.0).any():
        raise RuntimeError("a band of the invariant pixels is constant or uncorrelated between the dates: no regression line")
    gain = (syy - sxx + np.sqrt((syy - sxx) ** 2 + 4.0 * sxy ** 2)) / (2.0 * sxy)
    return gain, m.mean[c:] - gain * m.mean[:c], count


def class_transitions(map_a, map_b, num_classes, mask=None, ignore=None):
    """The from-to table of post-classification comparison: int64 [K + 1, K + 1] on the device, table[i, j] = the number of unmasked
    pixels of class i in ``map_a`` (any integer dtype) and class j in ``map_b`` (int64) of the same shape; index K collects the cells
    that hold no class in [0, K) (for ``map_a`` also the values of ``ignore``).  `scene_confusion` with map_a as the truth."""
    from .scene import scene_confusion
    if isinstance(map_a, torch.Tensor) and isinstance(map_b, torch.Tensor) and tuple(map_a.shape) != tuple(map_b.shape):
        raise RuntimeError(f"the two maps must have one shape, got {list(map_a.shape)} and {list(map_b.shape)}")
    return scene_confusion(map_b, map_a, num_classes, mask=mask, ignore=ignore)
