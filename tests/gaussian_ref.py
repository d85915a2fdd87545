"""NumPy float64 restatement of the Gaussian classifier (include/eae.h, "latent Gaussian models"; eae_amd.gaussian) and the bounds the
GPU tests compare with.  Nothing here is measured on the code under test: the bounds are derived from the fp32 format."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def finite_rows(z):
    return np.isfinite(np.asarray(z, dtype=np.float64)).all(axis=1)


def usable_labels(z, labels, k):
    """Labels with everything that is not summed turned into -1: values outside [0, k) and rows that hold a NaN or an Inf."""
    lab = np.asarray(labels).astype(np.int64).copy()
    lab[(lab < 0) | (lab >= k) | ~finite_rows(z)] = -1
    return lab


def moments_ref(z, labels, k):
    """(counts [K] int64, means [K, L] float64): a class without rows has mean 0."""
    z = np.asarray(z, dtype=np.float64)
    lab = usable_labels(z, labels, k)
    counts = np.zeros(k, dtype=np.int64)
    means = np.zeros((k, z.shape[1]))
    for q in range(k):
        m = lab == q
        counts[q] = int(m.sum())
        if counts[q]:
            means[q] = z[m].sum(0) / counts[q]
    return counts, means


def scatter_ref(z, labels, means32, k):
    """(S [K, L, L] float64, bound [K, L, L]) about the GIVEN fp32 means, as the kernel takes them: d = fl32(z - m) is one fp32
    subtraction, S_k = sum d d^T in float64 of those same d, and any fp32 summation order of n_k products, each rounded once, stays
    within (n_k + 2) 2^-24 sum |d_i d_j| of it.  Labels outside [0, k) are skipped; a class without rows gives 0 (and bound 0)."""
    z32 = np.asarray(z, dtype=np.float32)
    m32 = np.asarray(means32, dtype=np.float32)
    lab = np.asarray(labels)
    width = z32.shape[1]
    s = np.zeros((k, width, width))
    bound = np.zeros((k, width, width))
    for q in range(k):
        rows = lab == q
        nk = int(rows.sum())
        if nk:
            d = (z32[rows] - m32[q]).astype(np.float64)          # the fp32 difference, exactly
            s[q] = d.T @ d
            bound[q] = (nk + 2) * U * (np.abs(d).T @ np.abs(d))
    return s, bound


def shrink(cov, reg):
    return (1.0 - reg) * cov + reg * (np.trace(cov) / cov.shape[0]) * np.eye(cov.shape[0])


def fit_ref(counts, means, scatter, covariance="full", reg=1e-3, priors="empirical"):
    """(whiten [K or 1, L, L], offset [K], logdet [K]) in float64.  A class with fewer than 2 rows is absent (offset and logdet +inf,
    whiten 0, left out of the tied pool and of the priors' normalisation).  Sigma = C C^T, W = C^-T, logdet = 2 sum log diag C."""
    counts = np.asarray(counts, dtype=np.int64)
    s = np.asarray(scatter, dtype=np.float64)
    k, width = s.shape[0], s.shape[1]
    present = counts >= 2
    logdet = np.full(k, np.inf)

    def whitening(cov):
        c = np.linalg.cholesky(shrink(cov, reg))
        return np.linalg.inv(c).T, 2.0 * np.log(np.diag(c)).sum()

    if covariance == "full":
        whiten = np.zeros((k, width, width))
        for q in np.flatnonzero(present):
            whiten[q], logdet[q] = whitening(s[q] / (counts[q] - 1))
    else:
        whiten = np.zeros((1, width, width))
        if present.any():
            whiten[0], ld = whitening(s[present].sum(0) / (counts[present].sum() - present.sum()))
            logdet[present] = ld
    if isinstance(priors, str):
        pi = counts.astype(np.float64) if priors == "empirical" else np.ones(k)
    else:
        pi = np.asarray(priors, dtype=np.float64).copy()
    pi[~present] = 0.0
    if present.any():
        pi = pi / pi.sum()
    with np.errstate(divide="ignore"):
        offset = np.where(pi > 0, logdet - 2.0 * np.log(np.where(pi > 0, pi, 1.0)), np.inf)
    return whiten, offset, logdet


def score_ref(z, mu32, w32, offset32):
    """(score64 [N, K], d64 [N, K], labels [N], tau [N, K], tau_s [N, K]) of the model as the kernel holds it (fp32 mu, W, offset; W
    [K or 1, L, L]).  d = fl32(z - mu) is one fp32 subtraction; u_j = sum_l W_lj d_l and d64 = sum_j u_j^2 in float64 of those d.

    Bounds of any fp32 evaluation that rounds every product and every add once: e_j = (L + 2) 2^-24 sum_l |W_lj d_l| on u_j, hence
    tau = sum_j (2 |u_j| e_j + e_j^2) + (L + 2) 2^-24 sum_j u_j^2 on d; the score adds the offset with one more rounding:
    tau_s = tau + 2^-24 (|score64| + tau).  An offset of +inf marks an absent class: score +inf, never the argmin.  A row with a NaN or
    an Inf, or with no present class, gets label -1; a non-finite row's scores are NaN."""
    z32 = np.asarray(z, dtype=np.float32)
    mu32 = np.asarray(mu32, dtype=np.float32)
    w = np.asarray(w32, dtype=np.float64)
    off = np.asarray(offset32, dtype=np.float64)
    n, width = z32.shape
    k = mu32.shape[0]
    ok = finite_rows(z32)
    score = np.full((n, k), np.nan)
    d64 = np.full((n, k), np.nan)
    tau = np.full((n, k), np.nan)
    g = (width + 2) * U
    for q in range(k):                        # (class by class: no N x K x L temporary)
        wq = w[q if w.shape[0] > 1 else 0]
        d = (z32[ok] - mu32[q]).astype(np.float64)
        u = d @ wq
        e = g * (np.abs(d) @ np.abs(wq))
        d64[ok, q] = (u * u).sum(1)
        tau[ok, q] = (2.0 * np.abs(u) * e + e * e).sum(1) + g * d64[ok, q]
        score[ok, q] = d64[ok, q] + off[q]
    with np.errstate(invalid="ignore"):
        tau_s = tau + U * (np.where(np.isinf(score), 0.0, np.abs(score)) + tau)
    labels = np.full(n, -1, dtype=np.int64)
    some = ok & np.isfinite(np.where(np.isnan(score), np.inf, score)).any(axis=1)
    labels[some] = score[some].argmin(axis=1)
    return score, d64, labels, tau, tau_s


def accept(z, mu32, w32, offset32, labels, maha=None):
    """The acceptance rule, for every row, none left out: a chosen class's float64 score lies within tau_s(n, chosen) + tau_s(n, argmin)
    of the row's minimum; maha within tau(n, chosen) of the float64 distance (and >= 0); rows the reference labels -1 hold -1 and NaN.
    Returns score_ref's tuple."""
    ref = score_ref(z, mu32, w32, offset32)
    score, d64, lab_ref, tau, tau_s = ref
    labels = np.asarray(labels)
    ok = lab_ref >= 0
    assert np.array_equal(labels >= 0, ok) and (labels[~ok] == -1).all()
    rows = np.flatnonzero(ok)
    got, best = labels[rows], lab_ref[rows]
    assert ((got >= 0) & (got < score.shape[1])).all()
    assert np.isfinite(score[rows, got]).all()                                   # an absent class is never chosen
    assert (score[rows, got] - score[rows, best] <= tau_s[rows, got] + tau_s[rows, best]).all()
    if maha is not None:
        maha = np.asarray(maha)
        assert np.isnan(maha[~ok]).all()
        assert (maha[rows] >= 0).all() and (np.abs(maha[rows].astype(np.float64) - d64[rows, got]) <= tau[rows, got]).all()
    return ref


def blobs(n, width, k, seed, sep=4.0, spread=1.0):
    """Gaussian blobs with a covariance of their own each: centres of norm `sep`, row n in blob n % k, within a blob
    z = centre + spread / sqrt(L) * A_k g with A_k = I + 0.3 G_k / sqrt(L).  Returns (z fp32, blob ids int64)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, width))
    centres *= sep / np.linalg.norm(centres, axis=1, keepdims=True)
    mix = np.eye(width) + 0.3 * rng.standard_normal((k, width, width)) / np.sqrt(width)
    ids = np.arange(n) % k
    g = rng.standard_normal((n, width)) * (spread / np.sqrt(width))
    z = np.empty((n, width))
    for q in range(k):
        z[ids == q] = centres[q] + g[ids == q] @ mix[q]
    return z.astype(np.float32), ids.astype(np.int64)
