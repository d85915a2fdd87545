"""NumPy float64 restatement of change detection (eae_amd.change; include/eae.h, "change detection"), and the
planted-change scenes the tests share.  Everything here starts from the same fp32 pixel vector the kernels form, v = [a / div_a,
b / div_b] (one correctly rounded fp32 division per value), and the same fp32 differences d = v - pivot or v - mean; from there on it
is float64.

Error bounds, derived (u = 2^-24, the unit roundoff of fp32):

moments.  Within a chunk an accumulator adds at most n_chunk products w d_i d_j one after the other.  The product costs two roundings
  (w d_i, then the multiply-add's single rounding covers the second product and the add), a chain of n additions at most n more, so to
  first order |fp32 sum - exact sum| <= (n_chunk + 2) u sum w |d_i d_j| over the chunk's pixels; summing the chunks, each with the
  largest n_chunk (the plan's chunk size), gives (chunk + 2) u sum w |d_i d_j| over the raster.  s and N are the same chain with
  d_j = 1 and d_i = d_j = 1.  The float64 additions of the partials add at most G 2^-53 of the same sum: below the bound's last digit.

variates.  M_i is a chain of 2C fused multiply-adds: |M_i - exact| <= (2C + 1) u sum_j |T_ji d_j|.  Z = sum_i M_i^2 is a chain of C
  fmas over the computed M: |Z - exact| <= sum_i (2 |M_i| e_i + e_i^2) + (C + 1) u sum_i (|M_i| + e_i)^2 with e_i the bound of M_i.

prob.  The kernel's closed form is compared with this file's float64 closed form AT THE fp32 Z THE KERNEL WROTE, so only its
  evaluation is bounded here.  ULP figures of the HIP math API documentation: expf 1, erfcf 4, sqrtf 1 (an ulp is at most 2 u
  relative).  h = Z / 2 and h / 2 are exact.  Even dof = 2m: t_j = t_{j-1} (h / j) costs two roundings a term, the sum of m positive
  terms m - 1 more, the two factors e^(-h/2) 2 u each and their products 2 more: relative error <= (3 (m - 1) + 6) u.  Odd dof = 2m + 1:
  sqrt(h) carries 2 u, which erfc amplifies by y erfc'(y) / erfc(y) <= 2 h + 1.5 sqrt(h) (from erfc(y) > 2 e^(-y^2) / (sqrt(pi) (y +
  sqrt(y^2 + 2)))), plus erfcf's own 8 u; the series starts from sqrt(h) * fl(2 / sqrt(pi)) (4 u) and otherwise counts as the even one:
  (2 (m - 1) + (m - 1) + 4 + 6) u; the final addition 1 more.  All terms are positive, so the sum's relative error is at most the
  larger of the two plus u: (max(8 + 4 h + 3 sqrt(h), 3 m + 7) + 1) u.  Where the result or a term is not a normal fp32 number the
  error is absolute instead: 2^-126 is added (this also covers the kernel's return of 0 above Z = 256).  A factor 1.01 covers the
  second-order terms.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
SIGMA_FLOOR = 1e-6


# ---------------------------------------------------------------------------------------------------- pixels and validity
def chunk_pixels(c, h, w):
    """The moments kernel's chunk size: a function of (C, H, W) alone (C does not enter)."""
    per = -(-(h * w) // 4096)
    return max(256, -(-per // 256) * 256)


def pixel_vectors(a, b, div_a=1.0, div_b=1.0):
    """v float32 [2C, P]: the pixel vectors as the kernels form them."""
    c = a.shape[0]
    da = np.broadcast_to(np.asarray(div_a, dtype=np.float32).reshape(-1), (c,))
    db = np.broadcast_to(np.asarray(div_b, dtype=np.float32).reshape(-1), (c,))
    with np.errstate(all="ignore"):
        x = a.astype(np.float32).reshape(c, -1) / da[:, None]
        y = b.astype(np.float32).reshape(c, -1) / db[:, None]
    return np.concatenate([x, y]).astype(np.float32)


def _nodata_fires(s, nodata, rule):
    if nodata is None:
        return np.zeros(s.shape[1:], dtype=bool)
    m = np.isnan(s) if isinstance(nodata, float) and math.isnan(nodata) else s == nodata
    return m.all(0) if rule == "all" else m.any(0)


def valid_pixels(a, b, nodata_a=None, rule_a="all", nodata_b=None, rule_b="all", mask=None, weights=None):
    """bool [P]: the pixels that take part."""
    ok = ~(_nodata_fires(a, nodata_a, rule_a) | _nodata_fires(b, nodata_b, rule_b))
    for s in (a, b):
        if s.dtype == np.float32:
            ok &= np.isfinite(s).all(0)
    if mask is not None:
        ok &= mask == 0
    if weights is not None:
        with np.errstate(invalid="ignore"):
            ok &= (weights >= 0) & np.isfinite(weights)
    return ok.reshape(-1)


# ---------------------------------------------------------------------------------------------------- moments
def moments_ref(v, valid, pivot, weights, chunk):
    """(moments float64 [1 + 2C + (2C)^2], count, bound of the same shape) of eae_change_moments: v fp32 [2C, P], valid bool [P],
    pivot [2C] (rounded to fp32 as the call receives it), weights None or [P]."""
    n2 = v.shape[0]
    d = (v[:, valid] - np.asarray(pivot, dtype=np.float32)[:, None]).astype(np.float64)       # the fp32 difference, then float64
    w = np.ones(d.shape[1]) if weights is None else weights.reshape(-1)[valid].astype(np.float64)
    mom = np.concatenate([[w.sum()], d @ w, ((d * w) @ d.T).reshape(-1)])
    ad = np.abs(d)
    bound = (chunk + 2) * U * np.concatenate([[w.sum()], ad @ w, ((ad * w) @ ad.T).reshape(-1)])
    return mom, int(valid.sum()), bound


def mean_cov(mom, pivot, n2):
    n = mom[0]
    s = mom[1:1 + n2] / n
    return np.asarray(pivot, dtype=np.float32).astype(np.float64) + s, mom[1 + n2:].reshape(n2, n2) / n - np.outer(s, s)


# ---------------------------------------------------------------------------------------------------- the chi-square law
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def chi2_sf(dof, z):
    """Q(dof / 2, z / 2) in float64 for integer dof >= 1, elementwise: the closed forms of the header."""
    z = np.asarray(z, dtype=np.float64)
    h = 0.5 * np.maximum(z, 0.0)
    m = dof // 2
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if dof % 2:
            rt = np.sqrt(h)
            t = rt * (2.0 / math.sqrt(math.pi))
            s = np.zeros_like(h)
            for j in range(1, m + 1):
                if j > 1:
                    t = t * (h / (j - 0.5))
                s = s + t
            e = np.exp(-0.5 * h)
            out = _erfc(rt) + (s * e) * e
        else:
            t = np.ones_like(h)
            s = np.ones_like(h)
            for j in range(1, m):
                t = t * (h / j)
                s = s + t
            e = np.exp(-0.5 * h)
            out = (s * e) * e
    out = np.where(np.isnan(z), np.nan, np.where(np.isfinite(out), out, 0.0))
    return out


def chi2_isf(dof, p):
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


def prob_bound(dof, z):
    """The bound of |kernel prob - chi2_sf(dof, z)| for the fp32 z the kernel evaluated (module docstring)."""
    h = 0.5 * np.asarray(z, dtype=np.float64)
    m = dof // 2
    rel = np.maximum(8.0 + 4.0 * h + 3.0 * np.sqrt(h), 3.0 * m + 7.0) + 1.0 if dof % 2 else np.full_like(h, 3.0 * (m - 1) + 6.0)
    return 1.01 * rel * U * chi2_sf(dof, z) + TINY


# ---------------------------------------------------------------------------------------------------- the solve
def _inv_sqrt(s):
    lam, q = np.linalg.eigh(s)
    if not lam.min() > 0.0:
        raise np.linalg.LinAlgError("not positive definite")
    return (q / np.sqrt(lam)) @ q.T


def mad_ref(mean, cov, reg=0.0):
    """(rho descending, a, b, sigma): canonical correlations through the symmetric inverse square roots and an eigendecomposition
    (another route than the package's Cholesky + SVD), with the package's conventions: a^T Sxx a = b^T Syy b = 1, the sign that makes
    the largest-magnitude entry of Sxx a_i positive, sigma = max(sqrt(2 (1 - rho)), 1e-6)."""
    c = mean.shape[0] // 2
    sxx, syy, sxy = cov[:c, :c], cov[c:, c:], cov[:c, c:]
    sxx = (1.0 - reg) * sxx + reg * np.trace(sxx) / c * np.eye(c)
    syy = (1.0 - reg) * syy + reg * np.trace(syy) / c * np.eye(c)
    rx, ry = _inv_sqrt(sxx), _inv_sqrt(syy)
    k = rx @ sxy @ ry
    lam, u = np.linalg.eigh(k @ k.T)
    order = np.argsort(-lam)
    rho = np.sqrt(np.clip(lam[order], 0.0, 1.0))
    a = rx @ u[:, order]
    b = ry @ (k.T @ u[:, order]) / np.maximum(rho, 1e-300)
    t = sxx @ a
    sign = np.where(t[np.abs(t).argmax(0), np.arange(c)] < 0.0, -1.0, 1.0)
    return rho, a * sign, b * sign, np.maximum(np.sqrt(2.0 * (1.0 - rho)), SIGMA_FLOOR)


def variate_matrix(a, b, sigma):
    return np.concatenate([a / sigma, -b / sigma])


# ---------------------------------------------------------------------------------------------------- variates
def variates_ref(v, valid, mean, t, dof):
    """(M float64 [C, P], Z [P], prob [P], bound of M [C, P], bound of Z [P]) from the fp32 mean and T the call receives; NaN / 0 at
    the invalid pixels."""
    n2, p = v.shape
    c = n2 // 2
    mean = np.asarray(mean, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = (v - mean[:, None]).astype(np.float64)
    d[:, ~valid] = 0.0
    m = t.T @ d
    bm = (n2 + 1) * U * (np.abs(t).T @ np.abs(d))
    z = (m * m).sum(0)
    bz = (2.0 * np.abs(m) * bm + bm * bm).sum(0) + (c + 1) * U * ((np.abs(m) + bm) ** 2).sum(0)
    prob = chi2_sf(dof, z)
    m[:, ~valid] = np.nan
    z[~valid] = np.nan
    prob[~valid] = 0.0
    return m, z, prob, bm, bz


# ---------------------------------------------------------------------------------------------------- the iteration
def irmad_ref(a, b, iterations, div_a=1.0, div_b=1.0, valid=None, reg=0.0):
    """IR-MAD in float64 with the package's conventions, a fixed number of iterations: (history of rho, chi2 [P], prob [P], (mean, a,
    b, sigma) of the last model).  The float64 moments are exact sums about the mean's neighbourhood (the pivot is the first pixel
    mean), so this is the reference the fp32 kernels are measured against."""
    v = pixel_vectors(a, b, div_a, div_b).astype(np.float64)
    n2 = v.shape[0]
    c = n2 // 2
    ok = valid_pixels(a, b) if valid is None else valid
    w = ok.astype(np.float64)
    history = []
    for _ in range(iterations):
        n = w.sum()
        mean = (v[:, ok] @ w[ok]) / n
        d = v[:, ok] - mean[:, None]
        cov = (d * w[ok]) @ d.T / n
        rho, ca, cb, sigma = mad_ref(mean, cov, reg)
        history.append(rho)
        t = variate_matrix(ca, cb, sigma)
        z = np.full(v.shape[1], np.nan)
        z[ok] = ((t.T @ d) ** 2).sum(0)
        prob = np.where(ok, chi2_sf(c, z), 0.0)
        w = prob
    return history, z, prob, (mean, ca, cb, sigma)


def median_calibration(chi2, valid, dof, alpha):
    """(scale, change bool [P]): chi2 divided by median(chi2 over valid) / median of the chi-square law, tested at alpha."""
    scale = float(np.median(chi2[valid])) / chi2_isf(dof, 0.5)
    with np.errstate(invalid="ignore"):
        change = valid & (chi2_sf(dof, chi2 / scale) < alpha)
    return scale, change


def orthogonal_regression_ref(x, y):
    """(gain, offset) of the total-least-squares line y = gain x + offset of two float64 vectors: the major axis of their 2 x 2
    covariance from its eigenvectors."""
    mx, my = x.mean(), y.mean()
    cov = np.cov(np.stack([x, y]), bias=True)
    _, q = np.linalg.eigh(cov)
    gain = q[1, 1] / q[0, 1]
    return gain, my - gain * mx


# ---------------------------------------------------------------------------------------------------- planted-change scenes
BLOCK = (slice(30, 54), slice(40, 64))
GAINS = 0.8 + 0.05 * np.arange(4)


def planted(seed, dtype):
    """(a, b, changed bool [96, 96]): two C = 4, 96 x 96 scenes of ``dtype`` (np.uint16 or np.uint8).  A: four smooth sin / cos fields
    plus 0.5 N(0, 1), mixed by I + 0.4 N(0, 1), scaled to 500..3500 (20..220).  B = gain_c A + offset_c + N(0, 15 (1.5)), gain_c =
    0.8 + 0.05 c, offset_c = 100 + 30 c (10 + 3 c); the block rows 30:54, columns 40:64 of B is replaced by N(top / 2, top / 6),
    top = 3500 (220).  Both rounded and clipped to the dtype."""
    rng = np.random.default_rng(seed)
    h = w = 96
    lo, top, noise, off = (500.0, 3500.0, 15.0, 100.0 + 30.0 * np.arange(4)) if dtype == np.uint16 else \
        (20.0, 220.0, 1.5, 10.0 + 3.0 * np.arange(4))
    yy, xx = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    f = np.stack([np.sin(2 * np.pi * (rng.uniform(0.5, 2.5) * yy + rng.uniform())) * np.cos(2 * np.pi * (rng.uniform(0.5, 2.5) * xx
                                                                                                           + rng.uniform()))
                  for _ in range(4)])
    f = f + 0.5 * rng.standard_normal(f.shape)
    f = np.einsum("ij,jhw->ihw", np.eye(4) + 0.4 * rng.standard_normal((4, 4)), f)
    f = (f - f.min()) / (f.max() - f.min())
    a = lo + (top - lo) * f
    b = GAINS[:, None, None] * a + off[:, None, None] + noise * rng.standard_normal(a.shape)
    b[(slice(None),) + BLOCK] = rng.normal(top / 2, top / 6, size=(4, 24, 24))
    hi = np.iinfo(dtype).max
    changed = np.zeros((h, w), dtype=bool)
    changed[BLOCK] = True
    return np.clip(np.rint(a), 0, hi).astype(dtype), np.clip(np.rint(b), 0, hi).astype(dtype), changed
