"""NumPy float64 restatement of the nearest-neighbour search (include/eae.h, "latent neighbours") and of `knn_classify`'s votes, and
the acceptance check the GPU tests apply.  Nothing here is measured on the code under test: the bound is kmeans_ref.tau with the bank
in place of the centroids, derived from the fp32 format."""
import numpy as np

from kmeans_ref import finite_rows, tau

#          (Nq, M, L, k)
SHAPES = [(1, 1, 1, 1), (129, 33, 3, 32),
          (65, 31, 48, 32),              # M < k: the tail is -1 / NaN
          (300, 1031, 256, 7), (257, 300, 128, 32), (1000, 4096, 64, 10),
          (33, 70001, 64, 10),           # long bank, few queries: the bank is cut into slices
          (1, 5000, 64, 10)]
QUERY_TILE = 128                         # queries per workgroup of knn_search_kernel (LT_QT)
BOUNDARY_SHAPES = [(QUERY_TILE - 1, 200, 20, 5), (QUERY_TILE, 200, 20, 5), (QUERY_TILE + 1, 200, 20, 5),
                   (516 * QUERY_TILE - 48, 40, 8, 3)]      # 516 query tiles: more than 512 workgroups, more than one round of the device


def distances(q, bank):
    """d64 [Nq, M]: the float64 squared distances, row by row or column by column (no Nq x M x L temporary)."""
    q = np.asarray(q, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    d = np.empty((q.shape[0], bank.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        if q.shape[0] <= bank.shape[0]:
            for n in range(q.shape[0]):
                d[n] = ((bank - q[n]) ** 2).sum(1)
        else:
            for m in range(bank.shape[0]):
                d[:, m] = ((q - bank[m]) ** 2).sum(1)
    return d


def eligible(q, bank, self_offset=-1):
    """bool [Nq, M]: pair (n, m) may be returned: both rows finite, and m != n + self_offset when that is >= 0."""
    ok = finite_rows(q)[:, None] & finite_rows(bank)[None, :]
    if self_offset >= 0:
        n = np.arange(q.shape[0])
        m = n + self_offset
        keep = m < bank.shape[0]
        ok[n[keep], m[keep]] = False
    return ok


def knn_ref(q, bank, k, self_offset=-1):
    """(idx [Nq, k] int64, dist [Nq, k] float64, d64 [Nq, M] with +Inf at ineligible pairs): the k eligible bank rows with the
    smallest (d, m), ascending; -1 / NaN where fewer than k are eligible."""
    d = distances(q, bank)
    d[~eligible(q, bank, self_offset)] = np.inf
    dp = d if d.shape[1] >= k else np.concatenate([d, np.full((d.shape[0], k - d.shape[1]), np.inf)], axis=1)
    order = np.argsort(dp, axis=1, kind="stable")[:, :k]         # stable: ascending m among equal d
    dist = np.take_along_axis(dp, order, 1)
    idx = np.where(np.isinf(dist), -1, order).astype(np.int64)
    return idx, np.where(np.isinf(dist), np.nan, dist), d


def brute_force(q, bank, k, self_offset=-1):
    """The same by plain loops (for the reference's own test)."""
    q = np.asarray(q, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    idx = np.full((len(q), k), -1, dtype=np.int64)
    dist = np.full((len(q), k), np.nan)
    for n in range(len(q)):
        if not np.isfinite(q[n]).all():
            continue
        pairs = []
        for m in range(len(bank)):
            if np.isfinite(bank[m]).all() and not (self_offset >= 0 and m == n + self_offset):
                pairs.append((float(sum((q[n, l] - bank[m, l]) ** 2 for l in range(q.shape[1]))), m))
        pairs.sort()
        for j, (dd, m) in enumerate(pairs[:k]):
            idx[n, j], dist[n, j] = m, dd
    return idx, dist


def vote_ref(idx, dist, bank_labels, num_classes, weights="uniform"):
    """(labels [Nq] int64, votes [Nq, C] float64): a neighbour of -1 or with a label outside [0, C) casts no vote; uniform votes count,
    "distance" votes weigh 1 / (dist + 1e-12); the class with the most votes, the lowest id on a tie; -1 without a vote."""
    idx = np.asarray(idx)
    bank_labels = np.asarray(bank_labels)
    votes = np.zeros((idx.shape[0], num_classes))
    labels = np.full(idx.shape[0], -1, dtype=np.int64)
    for n in range(idx.shape[0]):
        cast = False
        for j in range(idx.shape[1]):
            if idx[n, j] < 0:
                continue
            c = int(bank_labels[idx[n, j]])
            if 0 <= c < num_classes:
                votes[n, c] += 1.0 if weights == "uniform" else 1.0 / (float(dist[n, j]) + 1e-12)
                cast = True
        if cast:
            labels[n] = int(np.argmax(votes[n]))                 # first maximum: the lowest class id
    return labels, votes


def bound(q, bank):
    """tau_n of every query row against the finite bank rows (NaN for a query row that is not finite)."""
    bank = np.asarray(bank)
    fin = finite_rows(bank)
    with np.errstate(invalid="ignore", over="ignore"):
        return tau(q, bank[fin] if fin.any() else np.zeros((1, bank.shape[1])))


def accept(q, bank, k, idx, dist=None, self_offset=-1):
    """Every row and every slot, none left out.  With d64 the float64 distances and s_j the j-th smallest eligible one of row n:
    |d64[n, idx[n, j]] - s_j| <= tau_n (each fp32 score is within tau / 2 of the truth and order statistics are 1-Lipschitz in the
    sup norm); indices distinct and eligible; slots beyond the number of eligible rows hold -1 / NaN, exactly those; dist is
    non-decreasing, >= 0 and within tau_n of d64.  Returns the reference (idx, dist, d64)."""
    ridx, rdist, d = knn_ref(q, bank, k, self_offset)
    t = bound(q, bank)
    nq = d.shape[0]
    assert idx.shape == (nq, k) and idx.dtype == np.int64
    filled = ridx >= 0
    assert np.array_equal(idx >= 0, filled), "the filled slots are not the reference's"
    assert (idx[~filled] == -1).all()
    assert (idx[filled] < d.shape[1]).all()
    got = np.where(filled, np.take_along_axis(d, np.maximum(idx, 0), 1), 0.0)
    assert np.isfinite(got).all(), "an ineligible bank row was returned"
    srt = np.sort(idx, axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any(), "a bank row was returned twice"
    want = np.where(filled, rdist, 0.0)
    tt = np.where(np.isnan(t), 0.0, t)[:, None]
    assert (np.abs(got - want) <= tt).all(), float((np.abs(got - want) / np.maximum(tt, 1e-300)).max())
    if dist is not None:
        assert dist.shape == (nq, k) and dist.dtype == np.float32
        assert np.isnan(dist[~filled]).all() and not np.isnan(dist[filled]).any()
        dd = np.where(filled, dist.astype(np.float64), 0.0)
        assert (dd >= 0).all()
        both = filled[:, 1:] & filled[:, :-1]
        assert (dd[:, 1:][both] >= dd[:, :-1][both]).all(), "dist decreases along a row"
        assert (np.abs(dd - got) <= tt).all(), float((np.abs(dd - got) / np.maximum(tt, 1e-300)).max())
    return ridx, rdist, d
