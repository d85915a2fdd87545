"""NumPy float64 restatement of the k-means kernels' semantics (include/eae.h, "latent clustering") and the bounds the GPU tests
compare with.  Nothing here is measured on the code under test: the bounds are derived from the fp32 format."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def finite_rows(z):
    return np.isfinite(np.asarray(z, dtype=np.float64)).all(axis=1)


def assign_ref(z, c):
    """(d64 [N, K], labels [N]): the full float64 squared-distance matrix and its argmin (first minimum: the lowest k on a tie).  A row
    with a NaN or an Inf gets label -1 and a NaN row of d64."""
    z = np.asarray(z, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    ok = finite_rows(z)
    d = np.full((z.shape[0], c.shape[0]), np.nan)
    for q in range(c.shape[0]):          # (column by column: no N x K x L temporary)
        d[ok, q] = ((z[ok] - c[q]) ** 2).sum(1)
    labels = np.full(z.shape[0], -1, dtype=np.int64)
    labels[ok] = d[ok].argmin(axis=1)
    return d, labels


def update_ref(z, labels, c):
    """(means [K, L] float64, counts [K] int64): the mean of the rows of each label in [0, K); an empty cluster keeps its row of c;
    labels outside [0, K) are skipped."""
    z = np.asarray(z, dtype=np.float64)
    labels = np.asarray(labels)
    out = np.asarray(c, dtype=np.float64).copy()
    k = out.shape[0]
    counts = np.zeros(k, dtype=np.int64)
    for q in range(k):
        m = labels == q
        counts[q] = int(m.sum())
        if counts[q]:
            out[q] = z[m].sum(0) / counts[q]
    return out, counts


def fit_ref(z, init, max_iter=100, tol=0.0, trace=None):
    """Lloyd's loop as `kmeans_fit` states it: assign; from the second pass on, with tol a number, stop when changed <= tol * N;
    update.  Ending by max_iter adds one final assign.  Returns (centroids, labels, d64, counts of the returned labels, n_iter).
    trace: a list that receives (z-vs-centroids d64, labels) of every assign along the trajectory."""
    c = np.asarray(init, dtype=np.float64).copy()
    n = z.shape[0]
    labels, n_iter, settled = None, 0, False
    for it in range(max_iter):
        d, new = assign_ref(z, c)
        if trace is not None:
            trace.append((d, new, c.copy()))
        changed = n if labels is None else int((new != labels).sum())
        labels = new
        if tol is not None and it > 0 and changed <= tol * n:
            settled = True
            break
        c, _ = update_ref(z, labels, c)
        n_iter += 1
    if not settled:
        d, labels = assign_ref(z, c)
        if trace is not None:
            trace.append((d, labels, c.copy()))
    counts = np.bincount(labels[labels >= 0], minlength=c.shape[0]).astype(np.int64)
    return c, labels, d, counts, n_iter


def tau(z, c):
    """The fp32 comparison bound of every row: tau_n = 4 (L + 2) 2^-24 (||z_n|| + max_k ||c_k||)^2.  Any fp32 summation order of L
    products has relative error <= gamma_L ~ L 2^-24 on sum |a b| <= ||z|| ||c||, the same holds for ||c||^2, two scores are compared
    (hence the doubling), and the final add contributes the + 2."""
    z = np.asarray(z, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    zn = np.sqrt((z ** 2).sum(1))
    cm = np.sqrt((c ** 2).sum(1)).max()
    return 4.0 * (z.shape[1] + 2) * U * (zn + cm) ** 2


def update_bound(z, labels, k):
    """[K, L]: (n_k + 1) 2^-24 sum_{n in k} |z_nl| / n_k, the order-free fp32 summation bound plus the division (inf where n_k = 0)."""
    z = np.abs(np.asarray(z, dtype=np.float64))
    out = np.full((k, z.shape[1]), np.inf)
    for q in range(k):
        m = labels == q
        nk = int(m.sum())
        if nk:
            out[q] = (nk + 1) * U * z[m].sum(0) / nk
    return out


def blobs(n, width, k, seed):
    """Well-separated blobs: centres of norm about 4, spread 0.05 / sqrt(L) per coordinate, row n in blob n % k.  Returns (z fp32,
    blob ids, init fp32 = the first row of each blob)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, width))
    centres *= 4.0 / np.linalg.norm(centres, axis=1, keepdims=True)
    ids = np.arange(n) % k
    z = (centres[ids] + rng.standard_normal((n, width)) * (0.05 / np.sqrt(width))).astype(np.float32)
    return z, ids, z[:k].copy()
